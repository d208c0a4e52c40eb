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
// Scalar block layout (32-bit words, one block per optimizer):
//   [0] float grad_norm   pre-clip global L2 norm (0 when clipping is off)
//   [1] float clip_coef   min(1, max_norm / (grad_norm + 1e-6)); 1 when off
//   [2] int   step        optimizer steps taken, counting the one in flight
//   [3]       reserved
//   [4+g] float lr of param group g
//
// Cross-block hand-off happens only over kernel boundaries on one stream:
// no block writes a word another block of the same launch reads, and there
// are no atomics, so every result is bit-reproducible run to run (float
// atomics are order-dependent) and eager and graph-replayed steps agree
// bit for bit.

#include "swq_common.h"

#define SWQ_SCALAR_GRAD_NORM 0
#define SWQ_SCALAR_CLIP_COEF 1
#define SWQ_SCALAR_STEP 2
#define SWQ_SCALAR_LR0 4

// ---------------------------------------------------------------------------
// per-chunk sum of squares.  lists: 0=src.  Plain store, no zeroing needed.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(BLOCK_THREADS)
swq_multi_tensor_sumsq_partials(const long long* meta, int num_tensors,
                                float* partials) {
    MetaView mv{meta, num_tensors, 1};
    const int t = mv.block_tensor(blockIdx.x);
    const int c = mv.block_chunk(blockIdx.x);
    const long long base = (long long)c * CHUNK_ELEMS;
    const int n = (int)min((long long)CHUNK_ELEMS, mv.numel(t) - base);
    const float* src = (const float*)mv.addr(0, t) + base;

    float acc = 0.0f;
    const int vec_n = n / 4;
    const float4* s4 = (const float4*)src;
    for (int i = threadIdx.x; i < vec_n; i += BLOCK_THREADS) {
        float4 s = s4[i];
        acc += s.x * s.x + s.y * s.y + s.z * s.z + s.w * s.w;
    }
    for (int i = vec_n * 4 + threadIdx.x; i < n; i += BLOCK_THREADS)
        acc += src[i] * src[i];

    const float total = block_reduce_sum(acc);
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
// host-side launchers (torch-independent; called from bindings.cpp).  They
// allocate nothing and synchronize nothing: the partials workspace and the
// scalar block are owned by the optimizer.  Grids are one block per chunk,
// as in fused_ops.hip.
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
