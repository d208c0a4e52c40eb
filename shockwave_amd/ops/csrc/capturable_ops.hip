// CDNA4 (gfx950 / MI355X) graph-safe fused optimizer kernels.
//
// The by-value kernels in fused_ops.hip take lr / step / buf_initialized
// as kernel arguments, so a captured hipGraph freezes them.  The kernels
// here read those scalars from a small device-resident block instead, and
// fold a global-norm gradient clip into the update:
//
//   swq_multi_tensor_sumsq_partials  one block per chunk, stores that
//                                    chunk's sum(g^2) to partials[block]
//   swq_optim_prologue               ONE block: sums all partials in a
//                                    fixed order, writes grad_norm and
//                                    clip_coef, advances the step counter
//   swq_fused_sgd_cap / _adam_cap    the update, with lr / step /
//                                    clip_coef loaded from the block and
//                                    the gradient scaled in registers
//
// The scalar block's layout is in swq_layout.h.
//
// Cross-block hand-off happens only over kernel boundaries on one stream:
// no block writes a word another block of the same launch reads, and there
// are no atomics, so every result is bit-reproducible run to run (float
// atomics are order-dependent) and eager and graph-replayed steps agree
// bit for bit.

#include "swq_common.h"

// ---------------------------------------------------------------------------
// per-chunk sum of squares.  lists: 0=src.  Plain store, no zeroing needed.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(BLOCK_THREADS)
swq_multi_tensor_sumsq_partials(const long long* meta, int num_tensors,
                                float* partials) {
    const float total = swq_chunk_sumsq(meta, num_tensors);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------
// one-block prologue: fixed-order sum of the partials of ALL param groups,
// then grad_norm, clip_coef (torch.nn.utils.clip_grad_norm_ formula) and the
// step advance.  num_partials == 0 (clipping off) only advances the step.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(BLOCK_THREADS)
swq_optim_prologue(const float* partials, int num_partials, float* scalars,
                   float max_norm, int clip) {
    float acc = 0.0f;
    for (int i = threadIdx.x; i < num_partials; i += BLOCK_THREADS)
        acc += partials[i];
    const float total = block_reduce_sum(acc);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(total);
        float coef = 1.0f;
        if (clip) coef = fminf(1.0f, max_norm / (norm + 1e-6f));
        scalars[SWQ_SCALAR_GRAD_NORM] = norm;
        scalars[SWQ_SCALAR_CLIP_COEF] = coef;
        int* step = (int*)scalars + SWQ_SCALAR_STEP;
        *step = *step + 1;
    }
}

// ---------------------------------------------------------------------------
// capturable SGD: swq_fused_sgd with lr / first-step flag / clip from the
// scalar block.  lists: 0=param, 1=grad (left unmodified), 2=momentum buffer
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(BLOCK_THREADS)
swq_fused_sgd_cap(const long long* meta, int num_tensors,
                  const float* __restrict__ scalars, int group,
                  float momentum, float dampening, float weight_decay,
                  int nesterov) {
    const float lr = scalars[SWQ_SCALAR_LR0 + group];
    const float coef = scalars[SWQ_SCALAR_CLIP_COEF];
    // the prologue already counted this step: step 1 is the first one,
    // i.e. zero steps were complete when it started (buf = d_p branch)
    const int buf_initialized =
        (((const int*)scalars)[SWQ_SCALAR_STEP] - 1) != 0;

    swq_sgd_chunk<true>(meta, num_tensors, lr, momentum, dampening,
                        weight_decay, nesterov, buf_initialized, coef);
}

// ---------------------------------------------------------------------------
// capturable Adam / AdamW: swq_fused_adam with lr / step / clip from the
// scalar block.  lists: 0=param, 1=grad (left unmodified), 2=exp_avg,
// 3=exp_avg_sq
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(BLOCK_THREADS)
swq_fused_adam_cap(const long long* meta, int num_tensors,
                   const float* __restrict__ scalars, int group, float beta1,
                   float beta2, float eps, float weight_decay, int adamw) {
    const float lr = scalars[SWQ_SCALAR_LR0 + group];
    const float coef = scalars[SWQ_SCALAR_CLIP_COEF];
    const int step = ((const int*)scalars)[SWQ_SCALAR_STEP];

    swq_adam_chunk<true>(meta, num_tensors, lr, beta1, beta2, eps,
                         weight_decay, step, adamw, coef);
}

// ---------------------------------------------------------------------------
// host-side launchers (prototypes in swq_layout.h; called from
// bindings.cpp).  Grids are one block per chunk, as in fused_ops.hip.
// ---------------------------------------------------------------------------
extern "C" {

void swq_launch_multi_tensor_sumsq_partials(const long long* meta,
                                            int num_tensors, int num_chunks,
                                            float* partials, void* stream) {
    hipLaunchKernelGGL(swq_multi_tensor_sumsq_partials, dim3(num_chunks),
                       dim3(BLOCK_THREADS), 0, (hipStream_t)stream, meta,
                       num_tensors, partials);
}

void swq_launch_optim_prologue(const float* partials, int num_partials,
                               float* scalars, float max_norm, int clip,
                               void* stream) {
    hipLaunchKernelGGL(swq_optim_prologue, dim3(1), dim3(BLOCK_THREADS), 0,
                       (hipStream_t)stream, partials, num_partials, scalars,
                       max_norm, clip);
}

void swq_launch_fused_sgd_cap(const long long* meta, int num_tensors,
                              int num_chunks, const float* scalars, int group,
                              float momentum, float dampening,
                              float weight_decay, int nesterov,
                              void* stream) {
    hipLaunchKernelGGL(swq_fused_sgd_cap, dim3(num_chunks),
                       dim3(BLOCK_THREADS), 0, (hipStream_t)stream, meta,
                       num_tensors, scalars, group, momentum, dampening,
                       weight_decay, nesterov);
}

void swq_launch_fused_adam_cap(const long long* meta, int num_tensors,
                               int num_chunks, const float* scalars,
                               int group, float beta1, float beta2, float eps,
                               float weight_decay, int adamw, void* stream) {
    hipLaunchKernelGGL(swq_fused_adam_cap, dim3(num_chunks),
                       dim3(BLOCK_THREADS), 0, (hipStream_t)stream, meta,
                       num_tensors, scalars, group, beta1, beta2, eps,
                       weight_decay, adamw);
}

}  // extern "C"
