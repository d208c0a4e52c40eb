// Layout constants and launcher prototypes shared by the swq_ kernels
// (fused_ops.hip, capturable_ops.hip) and their torch glue (bindings.cpp).
// Plain C/C++, no HIP include.  shockwave_amd/ops/__init__.py keeps its own
// copy of the constants for the CPU path and checks it against the ones
// bindings.cpp exports from here.

#pragma once

#define CHUNK_ELEMS 32768  // elements per block: grids are one block per chunk
#define BLOCK_THREADS 256

// Metadata layout in the int64 device buffer:
//   [0 .. NL*T)            : data pointers, list-major (addr[l*T + t])
//   [NL*T .. NL*T + T)     : numel per tensor
//   [NL*T + T .. +2*C)     : (tensor_idx, chunk_idx) per chunk
// where NL = number of tensor lists, T = tensor count, C = chunk count.

// Scalar block layout (32-bit words, one block per optimizer):
//   [0] float grad_norm   pre-clip global L2 norm (0 when clipping is off)
//   [1] float clip_coef   min(1, max_norm / (grad_norm + 1e-6)); 1 when off
//   [2] int   step        optimizer steps taken, counting the one in flight
//   [3]       reserved
//   [4+g] float lr of param group g
#define SWQ_SCALAR_GRAD_NORM 0
#define SWQ_SCALAR_CLIP_COEF 1
#define SWQ_SCALAR_STEP 2
#define SWQ_SCALAR_LR0 4

// Host-side launchers, defined next to their kernels: torch-independent,
// they allocate nothing and synchronize nothing (the partials workspace and
// the scalar block belong to the optimizer); `stream` is a hipStream_t.
// The .hip files see these prototypes too, so a definition that disagrees
// with its prototype does not compile.
#ifdef __cplusplus
extern "C" {
#endif
void swq_launch_fused_sgd(const long long* meta, int num_tensors,
                          int num_chunks, float lr, float momentum,
                          float dampening, float weight_decay, int nesterov,
                          int buf_initialized, void* stream);
void swq_launch_fused_adam(const long long* meta, int num_tensors,
                           int num_chunks, float lr, float beta1, float beta2,
                           float eps, float weight_decay, int step, int adamw,
                           void* stream);
void swq_launch_multi_tensor_accum(const long long* meta, int num_tensors,
                                   int num_chunks, float alpha, void* stream);
void swq_launch_multi_tensor_l2norm_sq(const long long* meta, int num_tensors,
                                       int num_chunks, float* out,
                                       void* stream);
void swq_launch_gns_window_stats(const long long* grad_ptrs, int window,
                                 long long n, float* out, void* stream);
void swq_launch_multi_tensor_sumsq_partials(const long long* meta,
                                            int num_tensors, int num_chunks,
                                            float* partials, void* stream);
void swq_launch_optim_prologue(const float* partials, int num_partials,
                               float* scalars, float max_norm, int clip,
                               void* stream);
void swq_launch_fused_sgd_cap(const long long* meta, int num_tensors,
                              int num_chunks, const float* scalars, int group,
                              float momentum, float dampening,
                              float weight_decay, int nesterov, void* stream);
void swq_launch_fused_adam_cap(const long long* meta, int num_tensors,
                               int num_chunks, const float* scalars,
                               int group, float beta1, float beta2, float eps,
                               float weight_decay, int adamw, void* stream);
#ifdef __cplusplus
}
#endif
