// Shared device-side pieces of the swq_ multi-tensor kernels: chunk
// metadata view, block reduction, and the per-element optimizer updates.
//
// The per-element updates live here so the by-value kernels
// (fused_ops.hip) and the capturable kernels (capturable_ops.hip), which
// read lr / step / clip_coef from device memory, run the SAME expression
// tree and cannot drift apart.

#pragma once

#include <hip/hip_runtime.h>

#define CHUNK_ELEMS 32768
#define BLOCK_THREADS 256
#define WAVE 64

// metadata layout in the int64 device buffer:
//   [0 .. NL*T)            : data pointers, list-major (addr[l*T + t])
//   [NL*T .. NL*T + T)     : numel per tensor
//   [NL*T + T .. +2*C)     : (tensor_idx, chunk_idx) per chunk
// where NL = number of tensor lists, T = tensor count, C = chunk count.

struct MetaView {
    const long long* buf;
    int num_tensors;
    int num_lists;
    __device__ inline void* addr(int list, int t) const {
        return (void*)buf[list * num_tensors + t];
    }
    __device__ inline long long numel(int t) const {
        return buf[num_lists * num_tensors + t];
    }
    __device__ inline int block_tensor(int b) const {
        return (int)buf[num_lists * num_tensors + num_tensors + 2 * b];
    }
    __device__ inline int block_chunk(int b) const {
        return (int)buf[num_lists * num_tensors + num_tensors + 2 * b + 1];
    }
};

// ---------------------------------------------------------------------------
// block-level sum reduction: wave shuffle then LDS
// ---------------------------------------------------------------------------
__device__ inline float block_reduce_sum(float v) {
    __shared__ float warp_sums[BLOCK_THREADS / WAVE];
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    if (lane == 0) warp_sums[wid] = v;
    __syncthreads();
    if (wid == 0) {
        v = (lane < BLOCK_THREADS / WAVE) ? warp_sums[lane] : 0.0f;
        #pragma unroll
        for (int off = (BLOCK_THREADS / WAVE) / 2; off > 0; off >>= 1)
            v += __shfl_down(v, off, WAVE);
    }
    return v;  // valid on thread 0
}


// The clip scale must stay a separate rounding step: fused into the
// following multiply-add it would change the result even at coef == 1.0,
// and the capturable kernels would no longer match the by-value ones.
__device__ inline float swq_clip_scale(float g, float coef) {
#pragma clang fp contract(off)
    return g * coef;
}

// ---------------------------------------------------------------------------
// SGD with momentum + weight decay over one chunk (torch.optim.SGD
// semantics).  lists: 0=param, 1=grad, 2=momentum buffer.
//   buf_initialized: 0 on the very first step (buf = d_p), 1 afterwards
//   kClip: multiply the gradient by coef in registers (the stored gradient
//   is left alone); kClip=false compiles to the plain update.
// ---------------------------------------------------------------------------
template <bool kClip>
__device__ inline void swq_sgd_chunk(const long long* meta, int num_tensors,
                                     float lr, float momentum,
                                     float dampening, float weight_decay,
                                     int nesterov, int buf_initialized,
                                     float coef) {
    MetaView mv{meta, num_tensors, 3};
    const int t = mv.block_tensor(blockIdx.x);
    const int c = mv.block_chunk(blockIdx.x);
    const long long base = (long long)c * CHUNK_ELEMS;
    const int n = (int)min((long long)CHUNK_ELEMS, mv.numel(t) - base);

    float* p = (float*)mv.addr(0, t) + base;
    const float* g = (const float*)mv.addr(1, t) + base;
    float* m = (float*)mv.addr(2, t) + base;

    const int vec_n = n / 4;
    float4* p4 = (float4*)p;
    const float4* g4 = (const float4*)g;
    float4* m4 = (float4*)m;

    for (int i = threadIdx.x; i < vec_n; i += BLOCK_THREADS) {
        float4 pv = p4[i];
        float4 gv = g4[i];
        float4 bv = m4[i];
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            float d_p = ((const float*)&gv)[k];
            if (kClip) d_p = swq_clip_scale(d_p, coef);
            float pk = ((const float*)&pv)[k];
            if (weight_decay != 0.0f) d_p += weight_decay * pk;
            float buf;
            if (momentum != 0.0f) {
                buf = buf_initialized
                          ? momentum * ((const float*)&bv)[k] + (1.0f - dampening) * d_p
                          : d_p;
                ((float*)&bv)[k] = buf;
                d_p = nesterov ? d_p + momentum * buf : buf;
            }
            ((float*)&pv)[k] = pk - lr * d_p;
        }
        p4[i] = pv;
        if (momentum != 0.0f) m4[i] = bv;
    }
    // scalar tail
    for (int i = vec_n * 4 + threadIdx.x; i < n; i += BLOCK_THREADS) {
        float d_p = g[i];
        if (kClip) d_p = swq_clip_scale(d_p, coef);
        float pk = p[i];
        if (weight_decay != 0.0f) d_p += weight_decay * pk;
        if (momentum != 0.0f) {
            float buf = buf_initialized
                            ? momentum * m[i] + (1.0f - dampening) * d_p
                            : d_p;
            m[i] = buf;
            d_p = nesterov ? d_p + momentum * buf : buf;
        }
        p[i] = pk - lr * d_p;
    }
}

// ---------------------------------------------------------------------------
// Adam / AdamW over one chunk (torch.optim.Adam semantics, L2-style weight
// decay unless adamw).  lists: 0=param, 1=grad, 2=exp_avg, 3=exp_avg_sq.
// kClip as above.
// ---------------------------------------------------------------------------
template <bool kClip>
__device__ inline void swq_adam_chunk(const long long* meta, int num_tensors,
                                      float lr, float beta1, float beta2,
                                      float eps, float weight_decay, int step,
                                      int adamw, float coef) {
    MetaView mv{meta, num_tensors, 4};
    const int t = mv.block_tensor(blockIdx.x);
    const int c = mv.block_chunk(blockIdx.x);
    const long long base = (long long)c * CHUNK_ELEMS;
    const int n = (int)min((long long)CHUNK_ELEMS, mv.numel(t) - base);

    float* p = (float*)mv.addr(0, t) + base;
    const float* g = (const float*)mv.addr(1, t) + base;
    float* m = (float*)mv.addr(2, t) + base;
    float* v = (float*)mv.addr(3, t) + base;

    const float bc1 = 1.0f - __powf(beta1, (float)step);
    const float bc2 = 1.0f - __powf(beta2, (float)step);
    const float step_size = lr / bc1;
    const float inv_sqrt_bc2 = rsqrtf(bc2);

    const int vec_n = n / 4;
    float4* p4 = (float4*)p;
    const float4* g4 = (const float4*)g;
    float4* m4 = (float4*)m;
    float4* v4 = (float4*)v;

    for (int i = threadIdx.x; i < vec_n; i += BLOCK_THREADS) {
        float4 pv = p4[i], gv = g4[i], mv_ = m4[i], vv = v4[i];
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = ((const float*)&pv)[k];
            float gk = ((const float*)&gv)[k];
            if (kClip) gk = swq_clip_scale(gk, coef);
            if (adamw) pk *= (1.0f - lr * weight_decay);
            else if (weight_decay != 0.0f) gk += weight_decay * pk;
            float mk = beta1 * ((const float*)&mv_)[k] + (1.0f - beta1) * gk;
            float vk = beta2 * ((const float*)&vv)[k] + (1.0f - beta2) * gk * gk;
            ((float*)&mv_)[k] = mk;
            ((float*)&vv)[k] = vk;
            float denom = sqrtf(vk) * inv_sqrt_bc2 + eps;
            ((float*)&pv)[k] = pk - step_size * mk / denom;
        }
        p4[i] = pv; m4[i] = mv_; v4[i] = vv;
    }
    for (int i = vec_n * 4 + threadIdx.x; i < n; i += BLOCK_THREADS) {
        float pk = p[i], gk = g[i];
        if (kClip) gk = swq_clip_scale(gk, coef);
        if (adamw) pk *= (1.0f - lr * weight_decay);
        else if (weight_decay != 0.0f) gk += weight_decay * pk;
        float mk = beta1 * m[i] + (1.0f - beta1) * gk;
        float vk = beta2 * v[i] + (1.0f - beta2) * gk * gk;
        m[i] = mk; v[i] = vk;
        p[i] = pk - step_size * mk / (sqrtf(vk) * inv_sqrt_bc2 + eps);
    }
}
