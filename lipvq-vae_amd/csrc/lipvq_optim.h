// lipvq_optim.h -- the tensor-list argument block of the optimizer launches, shared by lipvq_bwd.hip (lipvq_adamw_f32) and
// lipvq_optim.hip (lipvq_adam_f32, the gradient-norm launches).
#ifndef LIPVQ_OPTIM_H_
#define LIPVQ_OPTIM_H_
#include "lipvq_common.h"

#define LIPVQ_ADAMW_MAX 32
struct AdamwArgs {
    float* p[LIPVQ_ADAMW_MAX];
    const float* g[LIPVQ_ADAMW_MAX];
    float* m[LIPVQ_ADAMW_MAX];
    float* v[LIPVQ_ADAMW_MAX];
    float* step[LIPVQ_ADAMW_MAX];
    long long n[LIPVQ_ADAMW_MAX];
    int count;
};

// lipvq_bwd.hip: the first of AdamW's two launches (adamw_steps_kernel: step[t] += 1, bc[2t] = 1 - beta1^step,
// bc[2t + 1] = sqrt(1 - beta2^step)), for lipvq_adam_f32 to run the very same kernel
void lipvq_adamw_launch_steps(const AdamwArgs& a, double beta1, double beta2, float* bc, hipStream_t st);
#endif
