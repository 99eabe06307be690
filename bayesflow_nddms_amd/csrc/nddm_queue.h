// nddm_queue.h -- the index arithmetic of the simulator's two-ended chunk queue (nddm_sim.h: open_tiles).  A header of its own so
// that the host compiler can build it stand-alone (tests/test_queue_split_host.py drives it with random interleavings).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nddm {

// The queue is ONE 64-bit word: the chunks pulled from the front so far in its low half, those pulled from the back in its high
// half.  A pull is one atomic add of QUEUE_FRONT or QUEUE_BACK that returns the OLD word (F, B):
//   * it is valid iff F + B < n_chunks -- the chunks [0, F) and [n_chunks - B, n_chunks) are gone, so at least one is left;
//   * it then takes chunk F from the front, or chunk n_chunks - 1 - B from the back.
// The adds are totally ordered, so F + B of the old words runs through 0, 1, 2, ...: exactly the first n_chunks pulls are valid, the
// front ones take 0, 1, ... upwards, the back ones n_chunks - 1, ... downwards, and they stop where they meet -- every chunk is handed
// out exactly once, with no second atomic.  A pull that finds the queue dry still adds to its half: the halves do not overflow into
// each other (F <= n_chunks + the waves of the grid < 2^32; the host keeps n_chunks < 2^31).  Returns the chunk, or -1 (dry).
constexpr unsigned long long QUEUE_FRONT = 1ull, QUEUE_BACK = 1ull << 32;
__host__ __device__ inline long long queue_pull(unsigned long long old, int n_chunks, bool back)
{
    const unsigned long long f = old & 0xffffffffull, b = old >> 32;
    if (f + b >= (unsigned long long)(long long)n_chunks) return -1;
    return back ? (long long)n_chunks - 1 - (long long)b : (long long)f;
}

}  // namespace nddm
