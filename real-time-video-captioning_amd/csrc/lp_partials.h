// The merge of the vocabulary head's three per-tile partials into a row's log-sum-exp, shared by the selection kernels
// (select.hip: argmax_final, draft_accept, score_final, distill_final) and the top-k alternatives of a row (skinny.hip:
// head_topk_kernel): the one statement of the add order, so that every kernel that reports a log-probability of a row reports
// the same bits.
#pragma once
#include "common.h"

// Log-probability of the row's winner from the third partial of the vocabulary head (skinny.hip: sum[t] = sum of exp(logit -
// val[t]) over tile t): log_softmax(logits)[winner] = -log(sum_t sum[t] * exp(val[t] - M)), M = the row's maximum (the winner's
// logit), tiles without a logit above -inf skipped.  The order of the adds is fixed and does not depend on the rows beside this
// one: thread tid takes tiles tid, tid + 256, .. ascending, the xor butterfly 32 .. 1 inside the wave, then waves 0 .. 3 in that
// order.  Called by every thread (one barrier inside; ss = four words of LDS); thread 0's return value is the row's, -inf for a
// row with no logit above -inf (M = -inf).  The partials of a row are 3 x 7.6 KB at the GIT vocabulary: L2 resident.
// total (nullable; launch_distill_final): thread 0's also gets the merged sum itself, 0 for such a row.
__device__ __forceinline__ float lp_partials(const float* __restrict__ val, const float* __restrict__ sum, const size_t base,
                                             const int ntiles, const float M, float* ss, float* total = nullptr) {
    const int tid = threadIdx.x;
    float acc = 0.f;
    if (M != -INFINITY) {                                                  // (uniform: M comes from LDS)
        for (int i0 = tid; i0 < ntiles; i0 += 256 * 8) {
            float v8[8], s8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + 256 * u, ntiles - 1);
                v8[u] = val[base + i];
                s8[u] = sum[base + i];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)                                     // (+ 0.f leaves a sum of non-negative terms as it is)
                acc += (i0 + 256 * u < ntiles && v8[u] != -INFINITY) ? s8[u] * __expf(v8[u] - M) : 0.f;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((tid & 63) == 0) ss[tid >> 6] = acc;
    __syncthreads();
    if (M == -INFINITY) {
        if (total) *total = 0.f;
        return -INFINITY;
    }
    const float z = ((ss[0] + ss[1]) + ss[2]) + ss[3];
    if (total) *total = z;
    return -__logf(z);
}
