// The prompt of a forced selection, as argmax_final_kernel (select.hip) and beam_step_forced (search.hip) take it.  In an anonymous
// namespace like the kernels that carry it in their signatures: each of the two files has its own.
#pragma once
#include "common.h"

namespace {

// The prompt of a forced selection (gitcap_attach_prompt): ids int64 [rows][ld], lengths int32 [rows] (valid tokens, CLS included,
// clamped to [1, max_len] here: max_len <= ld is the host's check, so no read leaves a row), pos = the position the launch writes.
// <false> is empty: the launches without a prompt carry nothing.
template <bool FORCED> struct PromptSel {};
template <> struct PromptSel<true> { const int64_t* ids; const int32_t* lengths; int ld, max_len, pos; };
__device__ __forceinline__ int prompt_len(const int32_t* __restrict__ lengths, const int r, const int max_len) {
    return min(max(lengths[r], 1), max_len);
}

}  // namespace
