// What gitcap_distill (gitcap.hip) needs of a student handle, whose struct is private to student.hip: the checks of a
// teacher-forced pass, the pass itself up to its final LayerNorm rows, and the head weight those rows meet.  Not part of the C ABI.
#pragma once
#include "kernels.h"

#include <string>

struct gitcap_student;
struct StudentRows { const bf16_t* xb; HeadWeight head; };      // bf16 rows [rows * T][head.D] of the last pass
int student_device(const gitcap_student* h);
HeadWeight student_head_weight(const gitcap_student* h);         // (all null before the weights are finalized)
// gitcap_student_score's preconditions for rows x T positions from position 0; launches nothing.  0, or the code with `why` set.
int student_rows_check(const gitcap_student* h, int rows, int T, std::string& why);
// positions 0 .. T - 1 of `rows` rows through the decoder stack on s, no head; a failure leaves its message in `why` as well
int student_forward_rows(gitcap_student* h, const int64_t* ids, int ld_ids, int rows, int T, hipStream_t s, StudentRows* out, std::string& why);
