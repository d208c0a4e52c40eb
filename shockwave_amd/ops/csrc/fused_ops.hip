// CDNA4 (gfx950 / MI355X) fused multi-tensor kernels for the
// dynamic-adaptation hot path of the shockwave_amd runtime.
//
// Named requirements (BASELINE.json north star; reference call sites in
// SURVEY.md §2.4):
//   * fused SGD-momentum / Adam optimizer step   (#4)
//   * Accordion grad-accumulate + per-tensor L2 norm (#5)
//   * GNS window-average + norm estimator        (#6)
//
// Design notes:
//   * wave = 64 lanes; 256-thread blocks (4 waves per CU workgroup)
//   * all kernels are HBM-bound: float4 (16 B/lane) vectorized main loops,
//     grid built from 32K-element chunks so even an 11M-param model yields
//     ~340 workgroups (>256 CUs reachable)
//   * every chunked elementwise kernel is swq_chunk_for_each (swq_common.h)
//     plus one element functor
//   * reductions: 64-wide __shfl_down wave reduction -> LDS across the 4
//     waves -> ONE device-scope atomicAdd per block
//   * tensor/chunk metadata lives in a cached device buffer (no 4 KiB
//     kernel-arg limit, graph-capture safe: no allocation at launch time
//     once the cache is warm)
//
// Every kernel name is prefixed swq_ so rocprofv3 kernel traces attribute
// time unambiguously.

#include "swq_common.h"

// ---------------------------------------------------------------------------
// fused SGD with momentum + weight decay (torch.optim.SGD semantics)
//   lists: 0=param, 1=grad, 2=momentum buffer
//   buf_initialized: 0 on the very first step (buf = d_p), 1 afterwards
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(BLOCK_THREADS)
swq_fused_sgd(const long long* meta, int num_tensors, float lr,
              float momentum, float dampening, float weight_decay,
              int nesterov, int buf_initialized) {
    swq_sgd_chunk<false>(meta, num_tensors, lr, momentum, dampening,
                         weight_decay, nesterov, buf_initialized, 1.0f);
}

// ---------------------------------------------------------------------------
// fused Adam / AdamW (torch.optim.Adam semantics, L2-style weight decay)
//   lists: 0=param, 1=grad, 2=exp_avg, 3=exp_avg_sq
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(BLOCK_THREADS)
swq_fused_adam(const long long* meta, int num_tensors, float lr, float beta1,
               float beta2, float eps, float weight_decay, int step,
               int adamw) {
    swq_adam_chunk<false>(meta, num_tensors, lr, beta1, beta2, eps,
                          weight_decay, step, adamw, 1.0f);
}

// ---------------------------------------------------------------------------
// Accordion: multi-tensor accumulate  dst += src  (per-step grad accumulate)
//   lists: 0=dst(fp32 accumulator), 1=src(grad)
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(BLOCK_THREADS)
swq_multi_tensor_accum(const long long* meta, int num_tensors, float alpha) {
    swq_chunk_for_each<2>(meta, num_tensors, 0b01u,
                          [=](auto& e) { e[0] += alpha * e[1]; });
}

// ---------------------------------------------------------------------------
// Accordion: per-tensor squared L2 norms.  out[t] must be zeroed first.
//   lists: 0=src.  One atomicAdd per (block, tensor).
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(BLOCK_THREADS)
swq_multi_tensor_l2norm_sq(const long long* meta, int num_tensors,
                           float* out) {
    int t;
    const float total = swq_chunk_sumsq(meta, num_tensors, &t);
    if (threadIdx.x == 0) atomicAdd(&out[t], total);
}

// ---------------------------------------------------------------------------
// GNS estimator: window-average gradient norm + current gradient norm.
//
//   grads: W pointers to flat fp32 gradients of length n (the sliding
//   window; grads[W-1] = the current gradient).
//   out[0] += || (1/W) sum_w g_w ||^2    (big-batch norm estimate)
//   out[1] += || g_{W-1} ||^2            (small-batch norm)
// Zero out[0:2] before launch.  Grid-stride, one pass over all W grads
// (any W: the window is a runtime loop, per-lane accumulation in registers,
// 16 B loads per grad).  Not chunked: one flat buffer per gradient.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(BLOCK_THREADS)
swq_gns_window_stats(const long long* grad_ptrs, int window, long long n,
                     float* out) {
    float acc_big = 0.0f, acc_small = 0.0f;
    const float inv_w = 1.0f / (float)window;
    const long long vec_n = n / 4;
    const long long stride = (long long)gridDim.x * BLOCK_THREADS;
    const long long tid = (long long)blockIdx.x * BLOCK_THREADS + threadIdx.x;

    for (long long i = tid; i < vec_n; i += stride) {
        float4 mean = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 last;
        for (int w = 0; w < window; ++w) {
            const float4 g = ((const float4*)grad_ptrs[w])[i];
            mean.x += g.x; mean.y += g.y; mean.z += g.z; mean.w += g.w;
            if (w == window - 1) last = g;
        }
        mean.x *= inv_w; mean.y *= inv_w; mean.z *= inv_w; mean.w *= inv_w;
        acc_big += mean.x * mean.x + mean.y * mean.y + mean.z * mean.z
                 + mean.w * mean.w;
        acc_small += last.x * last.x + last.y * last.y + last.z * last.z
                   + last.w * last.w;
    }
    for (long long i = vec_n * 4 + tid; i < n; i += stride) {
        float mean = 0.0f, last = 0.0f;
        for (int w = 0; w < window; ++w) {
            const float g = ((const float*)grad_ptrs[w])[i];
            mean += g;
            if (w == window - 1) last = g;
        }
        mean *= inv_w;
        acc_big += mean * mean;
        acc_small += last * last;
    }

    const float big = block_reduce_sum(acc_big);
    __syncthreads();  // reuse of the reduction LDS between the two calls
    const float small_ = block_reduce_sum(acc_small);
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], big);
        atomicAdd(&out[1], small_);
    }
}

// ---------------------------------------------------------------------------
// host-side launchers (prototypes in swq_layout.h; called from bindings.cpp)
// ---------------------------------------------------------------------------
extern "C" {

void swq_launch_fused_sgd(const long long* meta, int num_tensors,
                          int num_chunks, float lr, float momentum,
                          float dampening, float weight_decay, int nesterov,
                          int buf_initialized, void* stream) {
    hipLaunchKernelGGL(swq_fused_sgd, dim3(num_chunks), dim3(BLOCK_THREADS), 0,
                       (hipStream_t)stream, meta, num_tensors, lr, momentum,
                       dampening, weight_decay, nesterov, buf_initialized);
}

void swq_launch_fused_adam(const long long* meta, int num_tensors,
                           int num_chunks, float lr, float beta1, float beta2,
                           float eps, float weight_decay, int step, int adamw,
                           void* stream) {
    hipLaunchKernelGGL(swq_fused_adam, dim3(num_chunks), dim3(BLOCK_THREADS),
                       0, (hipStream_t)stream, meta, num_tensors, lr, beta1,
                       beta2, eps, weight_decay, step, adamw);
}

void swq_launch_multi_tensor_accum(const long long* meta, int num_tensors,
                                   int num_chunks, float alpha, void* stream) {
    hipLaunchKernelGGL(swq_multi_tensor_accum, dim3(num_chunks),
                       dim3(BLOCK_THREADS), 0, (hipStream_t)stream, meta,
                       num_tensors, alpha);
}

void swq_launch_multi_tensor_l2norm_sq(const long long* meta, int num_tensors,
                                       int num_chunks, float* out,
                                       void* stream) {
    hipLaunchKernelGGL(swq_multi_tensor_l2norm_sq, dim3(num_chunks),
                       dim3(BLOCK_THREADS), 0, (hipStream_t)stream, meta,
                       num_tensors, out);
}

void swq_launch_gns_window_stats(const long long* grad_ptrs, int window,
                                 long long n, float* out, void* stream) {
    long long vec_n = n / 4;
    int blocks = (int)((vec_n + BLOCK_THREADS - 1) / BLOCK_THREADS);
    if (blocks > 2048) blocks = 2048;  // grid-stride past this
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(swq_gns_window_stats, dim3(blocks),
                       dim3(BLOCK_THREADS), 0, (hipStream_t)stream, grad_ptrs,
                       window, n, out);
}

}  // extern "C"
