// What csrc/train_quantile.hip (32-bit keys) and csrc/train_wquantile.hip (64-bit items: key << 32 | row) share: the order-preserving
// key of a float, the padded LDS image, the bitonic network walked three strides per LDS round trip -- templated on the item type I
// -- and the float64 position / interpolation steps.
//
// The LDS image is padded by 8 items per 64.  For 4-byte items (ds_read_b32 / ds_write_b32: 32 lanes a cycle, bank = dword mod 32)
// and for 8-byte items (ds_read_b64: 32 lanes a cycle over 64 banks, two banks a lane, so the slot is item mod 32; ds_write_b64: 16
// lanes a cycle over 32 banks, slot = item mod 16) the arithmetic is the same in ITEMS: the passes whose lowest stride is 8, 16 or
// 32 would put a cycle's lanes on 8, 16 or 32 items of one 32-item row; with the padding they fall on 32 (16) distinct slots.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace nddm_train {

__device__ __forceinline__ int q_phys(int i) { return i + ((i >> 6) << 3); }

// float -> key with the floats' order (finite values): negatives inverted, the others with the sign bit set.  -0 is taken as +0
// (the two compare equal; +0 is what comes back).  No finite value maps to 0xFFFFFFFF (that would be a NaN's bits).
__device__ __forceinline__ unsigned q_key(float v)
{
    unsigned u = __float_as_uint(v);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float q_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ __forceinline__ unsigned q_min(unsigned a, unsigned b) { return min(a, b); }
__device__ __forceinline__ unsigned q_max(unsigned a, unsigned b) { return max(a, b); }
__device__ __forceinline__ unsigned long long q_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long q_max(unsigned long long a, unsigned long long b) { return a < b ? b : a; }

// 8 contiguous items of the image (a padded block of 64 keeps them contiguous and 32-byte / 64-byte aligned), in 16-byte accesses
__device__ __forceinline__ void q_load8(const unsigned *p, unsigned (&v)[8], unsigned flip)
{
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    const uint4 a = q[0], b = q[1];
    v[0] = a.x ^ flip; v[1] = a.y ^ flip; v[2] = a.z ^ flip; v[3] = a.w ^ flip;
    v[4] = b.x ^ flip; v[5] = b.y ^ flip; v[6] = b.z ^ flip; v[7] = b.w ^ flip;
}

__device__ __forceinline__ void q_store8(unsigned *p, const unsigned (&v)[8], unsigned flip)
{
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(v[0] ^ flip, v[1] ^ flip, v[2] ^ flip, v[3] ^ flip);
    q[1] = make_uint4(v[4] ^ flip, v[5] ^ flip, v[6] ^ flip, v[7] ^ flip);
}

__device__ __forceinline__ void q_load8(const unsigned long long *p, unsigned long long (&v)[8], unsigned long long flip)
{
    const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const ulonglong2 a = q[e];
        v[2 * e] = a.x ^ flip;
        v[2 * e + 1] = a.y ^ flip;
    }
}

__device__ __forceinline__ void q_store8(unsigned long long *p, const unsigned long long (&v)[8], unsigned long long flip)
{
    ulonglong2 *q = reinterpret_cast<ulonglong2 *>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = make_ulonglong2(v[2 * e] ^ flip, v[2 * e + 1] ^ flip);
}

// ascending compare-exchanges of 2^NB items over their index bits NB-1 .. 0
template <typename I, int NB> __device__ __forceinline__ void q_network(I (&v)[8])
{
#pragma unroll
    for (int s = NB - 1; s >= 0; --s)
#pragma unroll
        for (int e = 0; e < (1 << NB); ++e)
            if (!(e & (1 << s))) {
                const I a = v[e], b = v[e | (1 << s)];
                v[e] = q_min(a, b);
                v[e | (1 << s)] = q_max(a, b);
            }
}

// the strides 2^(lb+NB-1) .. 2^lb of phase k (lb >= 3): a group is the 2^NB items that differ in those index bits; its direction is
// one bit of the index above them (descending = ascending on the inverted items)
template <typename I, int LOGN, int T, int NB> __device__ __forceinline__ void q_pass(I *keys, int lb, int k, int t)
{
    constexpr int G = (1 << LOGN) >> NB;
    for (int g = t; g < G; g += T) {
        const int base = ((g >> lb) << (lb + NB)) | (g & ((1 << lb) - 1));
        const I flip = (base & k) ? ~(I)0 : (I)0;
        I v[8];
#pragma unroll
        for (int e = 0; e < (1 << NB); ++e) v[e] = keys[q_phys(base + (e << lb))] ^ flip;
        q_network<I, NB>(v);
#pragma unroll
        for (int e = 0; e < (1 << NB); ++e) keys[q_phys(base + (e << lb))] = v[e] ^ flip;
    }
}

// the strides 4, 2, 1 of phase k >= 16 on 8 contiguous items
template <typename I, int LOGN, int T> __device__ __forceinline__ void q_pass_low(I *keys, int k, int t)
{
    constexpr int G = (1 << LOGN) >> 3;
    for (int g = t; g < G; g += T) {
        const I flip = ((g << 3) & k) ? ~(I)0 : (I)0;
        I v[8];
        q_load8(keys + q_phys(g << 3), v, flip);
        q_network<I, 3>(v);
        q_store8(keys + q_phys(g << 3), v, flip);
    }
}

// the phases k = 2, 4, 8 whole, on 8 contiguous items
template <typename I, int LOGN, int T> __device__ __forceinline__ void q_pass_first(I *keys, int t)
{
    constexpr int G = (1 << LOGN) >> 3;
    for (int g = t; g < G; g += T) {
        I v[8];
        q_load8(keys + q_phys(g << 3), v, (I)0);
#pragma unroll
        for (int m = 1; m <= 3; ++m)
#pragma unroll
            for (int s = m - 1; s >= 0; --s)
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (!(e & (1 << s))) {
                        const bool desc = (((g << 3) | e) & (1 << m)) != 0;
                        const I x = v[e], y = v[e | (1 << s)];
                        v[e] = desc ? q_max(x, y) : q_min(x, y);
                        v[e | (1 << s)] = desc ? q_min(x, y) : q_max(x, y);
                    }
        q_store8(keys + q_phys(g << 3), v, (I)0);
    }
}

// the whole sort of 2^LOGN items in the padded image, ascending; every thread of the workgroup calls it (it synchronises), the items
// written and a barrier passed before
template <typename I, int LOGN, int T> __device__ __forceinline__ void q_sort(I *keys, int t)
{
    q_pass_first<I, LOGN, T>(keys, t);
    __syncthreads();
#pragma unroll 1
    for (int m = 4; m <= LOGN; ++m) {
        const int k = 1 << m;                                 // (the last phase: no index has that bit, all ascending)
        int u = m - 3;                                        // the strides 2^(m-1) .. 8: index bits 3 .. 3 + u - 1, from the top
        for (; u >= 3; u -= 3) {
            q_pass<I, LOGN, T, 3>(keys, u, k, t);
            __syncthreads();
        }
        if (u == 2) q_pass<I, LOGN, T, 2>(keys, 3, k, t);
        if (u == 1) q_pass<I, LOGN, T, 1>(keys, 3, k, t);
        if (u) __syncthreads();
        q_pass_low<I, LOGN, T>(keys, k, t);
        __syncthreads();
    }
}

// h = (n - 1) p, j = floor(h), g = h - j;  a + (b - a) g: every operation rounded on its own (no contraction into an fma)
__device__ __forceinline__ double q_position(int n, double p, int &j)
{
#pragma clang fp contract(off)
    const double h = (double)(n - 1) * p;
    const double f = floor(h);
    j = (int)f;
    return h - f;
}

__device__ __forceinline__ double q_lerp(double a, double b, double g)
{
#pragma clang fp contract(off)
    const double d = b - a;
    const double m = d * g;
    return a + m;
}

}  // namespace nddm_train
