// The quantisation of a log weight, shared by every kernel that defines its result on INTEGER weights (csrc/train_wquantile.hip: the
// weighted quantiles; csrc/train_resample.hip: the resampling): with m the largest finite log_w of the set, W = rint(exp(log_w - m)
// 2^36), 0 where log_w is not finite, so 0 <= W <= 2^36.  One function, inlined wherever a weight is needed: the same instructions,
// the same bits, in either kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace nddm_train {

__device__ __forceinline__ long long wq_weight(double lw, double m)
{
    return isfinite(lw) ? (long long)rint(exp(lw - m) * 68719476736.0) : 0LL;
}

}  // namespace nddm_train
