// Shared device-side pieces of the swq_ multi-tensor kernels: chunk
// metadata view, block reduction, the chunk walker and the per-element
// optimizer updates.
//
// Every elementwise kernel is the walker plus ONE element functor, so an
// update is written once for the float4 main loop and the scalar tail, and
// once for the by-value kernels (fused_ops.hip) and the capturable kernels
// (capturable_ops.hip), which read lr / step / clip_coef from device
// memory: they run the SAME expression tree and cannot drift apart.

#pragma once

#include <hip/hip_runtime.h>

#include "swq_layout.h"

#define WAVE 64

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

// ---------------------------------------------------------------------------
// the block's chunk of NL tensor lists, read from the metadata buffer
// (layout in swq_layout.h): tensor index, element count and a pointer per
// list to the chunk's first element
// ---------------------------------------------------------------------------
template <int NL>
struct Chunk {
    int t;
    int n;
    float* ptr[NL];
    __device__ inline Chunk(const long long* meta, int num_tensors) {
        const long long* numel = meta + NL * num_tensors;
        const long long* chunks = numel + num_tensors;
        t = (int)chunks[2 * blockIdx.x];
        const long long base =
            (long long)(int)chunks[2 * blockIdx.x + 1] * CHUNK_ELEMS;
        n = (int)min((long long)CHUNK_ELEMS, numel[t] - base);
        #pragma unroll
        for (int l = 0; l < NL; ++l)
            ptr[l] = (float*)meta[l * num_tensors + t] + base;
    }
};

// The tail's view of one element: e[l] is the element of list l in memory,
// loaded where the functor reads it and stored where it assigns it.  Not a
// register copy: with the loads hoisted out of the functor hipcc contracts
// Adam's tail differently and its results move (see swq_adam_chunk).
template <int NL>
struct MemElems {
    float* const* ptr;
    int i;
    __device__ inline float& operator[](int l) const { return ptr[l][i]; }
};

// The chunk walker.  For every element of the block's chunk, f(e) sees
// e[l] = the element of list l and may assign it.  float4 main loop, where
// e is a register copy and the lists whose bit is set in store_mask are
// written back (the others are only read); then the same functor over the
// scalar tail, on memory directly.  f must assign exactly the lists in
// store_mask, or the two loops disagree.
template <int NL, typename F>
__device__ inline void swq_chunk_for_each(const long long* meta,
                                          int num_tensors,
                                          unsigned store_mask, F f) {
    const Chunk<NL> ck(meta, num_tensors);
    const int vec_n = ck.n / 4;
    for (int i = threadIdx.x; i < vec_n; i += BLOCK_THREADS) {
        float4 v[NL];
        #pragma unroll
        for (int l = 0; l < NL; ++l) v[l] = ((const float4*)ck.ptr[l])[i];
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            float e[NL];
            #pragma unroll
            for (int l = 0; l < NL; ++l) e[l] = ((const float*)&v[l])[k];
            f(e);
            #pragma unroll
            for (int l = 0; l < NL; ++l) ((float*)&v[l])[k] = e[l];
        }
        #pragma unroll
        for (int l = 0; l < NL; ++l)
            if (store_mask >> l & 1) ((float4*)ck.ptr[l])[i] = v[l];
    }
    for (int i = vec_n * 4 + threadIdx.x; i < ck.n; i += BLOCK_THREADS) {
        const MemElems<NL> e{ck.ptr, i};
        f(e);
    }
}

// Reading variant: sum of squares of the block's chunk of list 0 (the only
// list), block total valid on thread 0.  Per thread: vector loop, then
// tail, then the block reduction.  *t_out, if given, receives the tensor
// index.
__device__ inline float swq_chunk_sumsq(const long long* meta,
                                        int num_tensors,
                                        int* t_out = nullptr) {
    const Chunk<1> ck(meta, num_tensors);
    const auto sq = [](float x) { return x * x; };
    float acc = 0.0f;
    const int vec_n = ck.n / 4;
    for (int i = threadIdx.x; i < vec_n; i += BLOCK_THREADS) {
        const float4 s = ((const float4*)ck.ptr[0])[i];
        acc += sq(s.x) + sq(s.y) + sq(s.z) + sq(s.w);
    }
    for (int i = vec_n * 4 + threadIdx.x; i < ck.n; i += BLOCK_THREADS)
        acc += sq(ck.ptr[0][i]);
    if (t_out) *t_out = ck.t;
    return block_reduce_sum(acc);
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
// semantics).  lists: 0=param, 1=grad, 2=momentum buffer (written only
// when momentum != 0).
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
    swq_chunk_for_each<3>(
        meta, num_tensors, momentum != 0.0f ? 0b101u : 0b001u,
        [=](auto& e) {
            float d_p = e[1];
            if (kClip) d_p = swq_clip_scale(d_p, coef);
            const float pk = e[0];
            if (weight_decay != 0.0f) d_p += weight_decay * pk;
            if (momentum != 0.0f) {
                const float buf =
                    buf_initialized
                        ? momentum * e[2] + (1.0f - dampening) * d_p
                        : d_p;
                e[2] = buf;
                d_p = nesterov ? d_p + momentum * buf : buf;
            }
            e[0] = pk - lr * d_p;
        });
}

// ---------------------------------------------------------------------------
// Adam / AdamW over one chunk (torch.optim.Adam semantics, L2-style weight
// decay unless adamw).  lists: 0=param, 1=grad, 2=exp_avg, 3=exp_avg_sq.
// kClip as above.
//
// hipcc contracts this update differently in the float4 loop and in the
// tail (the tail's exp_avg_sq stays mul + mul + add), so up to three
// elements per tensor round differently from the rest; it has since the
// kernel was written, and results are kept bit for bit.
// scripts/kernel_digests.py shows whether an edit here moves them.
// ---------------------------------------------------------------------------
template <bool kClip>
__device__ inline void swq_adam_chunk(const long long* meta, int num_tensors,
                                      float lr, float beta1, float beta2,
                                      float eps, float weight_decay, int step,
                                      int adamw, float coef) {
    const float bc1 = 1.0f - __powf(beta1, (float)step);
    const float bc2 = 1.0f - __powf(beta2, (float)step);
    const float step_size = lr / bc1;
    const float inv_sqrt_bc2 = rsqrtf(bc2);

    swq_chunk_for_each<4>(meta, num_tensors, 0b1101u, [=](auto& e) {
        float pk = e[0], gk = e[1];
        if (kClip) gk = swq_clip_scale(gk, coef);
        if (adamw) pk *= (1.0f - lr * weight_decay);
        else if (weight_decay != 0.0f) gk += weight_decay * pk;
        const float mk = beta1 * e[2] + (1.0f - beta1) * gk;
        const float vk = beta2 * e[3] + (1.0f - beta2) * gk * gk;
        e[2] = mk;
        e[3] = vk;
        e[0] = pk - step_size * mk / (sqrtf(vk) * inv_sqrt_bc2 + eps);
    });
}
