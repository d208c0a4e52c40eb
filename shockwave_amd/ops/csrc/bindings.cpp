// Torch glue for the CDNA4 fused multi-tensor kernels (fused_ops.hip,
// capturable_ops.hip).
//
// Responsibilities:
//   * validate tensor lists (fp32, contiguous, same device)
//   * build + cache the int64 metadata buffer (pointers, numels,
//     chunk->tensor map) on device; cache key = the pointer/numel multiset,
//     so steady-state training steps perform NO host->device traffic and
//     are hipGraph-capture safe
//   * launch through the extern "C" launchers compiled by hipcc
//     (prototypes and layout constants: swq_layout.h)

#include <torch/extension.h>

#include <ATen/hip/HIPContext.h>

#include <map>
#include <vector>

#include "swq_layout.h"

namespace {

struct MetaEntry {
    torch::Tensor device_buf;
    int num_chunks;
    const long long* ptr() const {
        return (const long long*)device_buf.data_ptr<int64_t>();
    }
};

using Key = std::vector<long long>;
using Lists = std::vector<std::vector<torch::Tensor>>;
std::map<Key, MetaEntry> g_meta_cache;

void check_lists(const Lists& lists) {
    TORCH_CHECK(!lists.empty() && !lists[0].empty(), "empty tensor lists");
    const size_t T = lists[0].size();
    for (const auto& list : lists) {
        TORCH_CHECK(list.size() == T, "tensor list length mismatch");
        for (size_t t = 0; t < T; ++t) {
            const auto& ten = list[t];
            TORCH_CHECK(ten.is_cuda(), "swq ops require device tensors");
            TORCH_CHECK(ten.scalar_type() == torch::kFloat32,
                        "swq ops are fp32-only (got ", ten.scalar_type(), ")");
            // flat elementwise kernels: any dense non-overlapping layout is
            // fine (NCHW-contiguous or channels_last) as long as every list
            // shares the layout per tensor index
            TORCH_CHECK(ten.is_non_overlapping_and_dense(),
                        "tensor ", t, " not dense");
            TORCH_CHECK(ten.numel() == lists[0][t].numel(),
                        "numel mismatch across lists at tensor ", t);
            // layouts must agree so the flat kernels pair elements
            // correctly; strides of size-1 dims are don't-care (a 1x1
            // conv's NCHW-contiguous grad is layout-equal to its
            // channels_last param even though the stride tuples differ)
            const auto& ref = lists[0][t];
            for (int64_t d = 0; d < ten.dim(); ++d) {
                if (ten.size(d) <= 1) continue;
                TORCH_CHECK(ten.stride(d) == ref.stride(d),
                            "stride/layout mismatch across lists at tensor ",
                            t, " dim ", d);
            }
        }
    }
}

// upload `host` to `device` and cache it under `key`
const MetaEntry& upload_meta(Key key, std::vector<long long> host,
                             int num_chunks, const torch::Device& device) {
    auto cpu = torch::from_blob(host.data(), {(long long)host.size()},
                                torch::kInt64)
                   .clone();
    auto dev = cpu.to(device, /*non_blocking=*/false);
    return g_meta_cache.emplace(std::move(key), MetaEntry{dev, num_chunks})
        .first->second;
}

const MetaEntry& get_meta(const Lists& lists) {
    const int T = (int)lists[0].size();
    // pointers, then numels: the cache key, and the head of the buffer
    Key key;
    key.reserve(lists.size() * T + T);
    for (const auto& list : lists)
        for (const auto& ten : list)
            key.push_back((long long)ten.data_ptr());
    for (const auto& ten : lists[0]) key.push_back(ten.numel());

    auto it = g_meta_cache.find(key);
    if (it != g_meta_cache.end()) return it->second;

    // append the chunk map
    std::vector<long long> host = key;
    int num_chunks = 0;
    for (int t = 0; t < T; ++t) {
        const long long n = lists[0][t].numel();
        const int chunks = (int)((n + CHUNK_ELEMS - 1) / CHUNK_ELEMS);
        for (int c = 0; c < chunks; ++c) {
            host.push_back(t);
            host.push_back(c);
            ++num_chunks;
        }
    }
    return upload_meta(std::move(key), std::move(host), num_chunks,
                       lists[0][0].device());
}

void* current_stream(const torch::Tensor& ref) {
    return (void*)at::hip::getCurrentHIPStream(ref.device().index()).stream();
}

}  // namespace

void fused_sgd(std::vector<torch::Tensor> params,
               std::vector<torch::Tensor> grads,
               std::vector<torch::Tensor> momentum_bufs, double lr,
               double momentum, double dampening, double weight_decay,
               bool nesterov, bool buf_initialized) {
    Lists lists{params, grads, momentum_bufs};
    check_lists(lists);
    const auto& meta = get_meta(lists);
    swq_launch_fused_sgd(meta.ptr(), (int)params.size(), meta.num_chunks,
                         (float)lr, (float)momentum, (float)dampening,
                         (float)weight_decay, nesterov ? 1 : 0,
                         buf_initialized ? 1 : 0, current_stream(params[0]));
}

void fused_adam(std::vector<torch::Tensor> params,
                std::vector<torch::Tensor> grads,
                std::vector<torch::Tensor> exp_avgs,
                std::vector<torch::Tensor> exp_avg_sqs, double lr,
                double beta1, double beta2, double eps, double weight_decay,
                int64_t step, bool adamw) {
    Lists lists{params, grads, exp_avgs, exp_avg_sqs};
    check_lists(lists);
    const auto& meta = get_meta(lists);
    swq_launch_fused_adam(meta.ptr(), (int)params.size(), meta.num_chunks,
                          (float)lr, (float)beta1, (float)beta2, (float)eps,
                          (float)weight_decay, (int)step, adamw ? 1 : 0,
                          current_stream(params[0]));
}

void multi_tensor_accum(std::vector<torch::Tensor> dsts,
                        std::vector<torch::Tensor> srcs, double alpha) {
    Lists lists{dsts, srcs};
    check_lists(lists);
    const auto& meta = get_meta(lists);
    swq_launch_multi_tensor_accum(meta.ptr(), (int)dsts.size(),
                                  meta.num_chunks, (float)alpha,
                                  current_stream(dsts[0]));
}

torch::Tensor multi_tensor_l2norm_sq(std::vector<torch::Tensor> tensors,
                                     torch::Tensor out) {
    Lists lists{tensors};
    check_lists(lists);
    TORCH_CHECK(out.numel() == (long long)tensors.size(),
                "out must have one element per tensor");
    TORCH_CHECK(out.scalar_type() == torch::kFloat32 && out.is_cuda());
    out.zero_();
    const auto& meta = get_meta(lists);
    swq_launch_multi_tensor_l2norm_sq(meta.ptr(), (int)tensors.size(),
                                      meta.num_chunks, out.data_ptr<float>(),
                                      current_stream(tensors[0]));
    return out;
}

torch::Tensor gns_window_stats(std::vector<torch::Tensor> grads,
                               torch::Tensor out) {
    check_lists({grads});
    const long long n = grads[0].numel();
    for (const auto& g : grads) TORCH_CHECK(g.numel() == n);
    TORCH_CHECK(out.numel() >= 2 && out.is_cuda() &&
                out.scalar_type() == torch::kFloat32);
    out.zero_();

    // the buffer is the W pointers; the key adds n
    std::vector<long long> ptrs;
    for (const auto& g : grads) ptrs.push_back((long long)g.data_ptr());
    Key key = ptrs;
    key.push_back(n);
    auto it = g_meta_cache.find(key);
    const MetaEntry& meta =
        it != g_meta_cache.end()
            ? it->second
            : upload_meta(std::move(key), std::move(ptrs), 0,
                          grads[0].device());
    swq_launch_gns_window_stats(meta.ptr(), (int)grads.size(), n,
                                out.data_ptr<float>(),
                                current_stream(grads[0]));
    return out;
}

// ---------------------------------------------------------------------------
// capturable optimizers (capturable_ops.hip): scalars live in `scalars`, a
// device fp32 block owned by the optimizer (layout in swq_layout.h)
// ---------------------------------------------------------------------------

namespace {

void check_scalars(const torch::Tensor& scalars, int64_t group,
                   const torch::Tensor& ref) {
    TORCH_CHECK(scalars.is_cuda() && scalars.device() == ref.device(),
                "scalar block must live on the params' device");
    TORCH_CHECK(scalars.scalar_type() == torch::kFloat32 &&
                    scalars.is_contiguous(),
                "scalar block must be contiguous fp32");
    TORCH_CHECK(group >= 0 && scalars.numel() > SWQ_SCALAR_LR0 + group,
                "scalar block too small for param group ", group);
}

void check_partials(const torch::Tensor& partials, const torch::Tensor& ref) {
    TORCH_CHECK(partials.is_cuda() && partials.device() == ref.device() &&
                    partials.scalar_type() == torch::kFloat32 &&
                    partials.is_contiguous(),
                "partials must be a contiguous fp32 device tensor");
}

}  // namespace

int64_t multi_tensor_sumsq_partials(std::vector<torch::Tensor> tensors,
                                    torch::Tensor partials, int64_t offset) {
    Lists lists{tensors};
    check_lists(lists);
    const auto& meta = get_meta(lists);
    check_partials(partials, tensors[0]);
    TORCH_CHECK(offset >= 0 && offset + meta.num_chunks <= partials.numel(),
                "partials workspace too small: need ",
                offset + meta.num_chunks, ", have ", partials.numel());
    swq_launch_multi_tensor_sumsq_partials(
        meta.ptr(), (int)tensors.size(), meta.num_chunks,
        partials.data_ptr<float>() + offset, current_stream(tensors[0]));
    return meta.num_chunks;
}

void optim_prologue(torch::Tensor partials, int64_t num_partials,
                    torch::Tensor scalars, double max_norm, bool clip) {
    check_scalars(scalars, 0, scalars);
    check_partials(partials, scalars);
    TORCH_CHECK(num_partials >= 0 && num_partials <= partials.numel(),
                "num_partials out of range");
    swq_launch_optim_prologue(partials.data_ptr<float>(), (int)num_partials,
                              scalars.data_ptr<float>(), (float)max_norm,
                              clip ? 1 : 0, current_stream(scalars));
}

void fused_sgd_cap(std::vector<torch::Tensor> params,
                   std::vector<torch::Tensor> grads,
                   std::vector<torch::Tensor> momentum_bufs,
                   torch::Tensor scalars, int64_t group, double momentum,
                   double dampening, double weight_decay, bool nesterov) {
    Lists lists{params, grads, momentum_bufs};
    check_lists(lists);
    check_scalars(scalars, group, params[0]);
    const auto& meta = get_meta(lists);
    swq_launch_fused_sgd_cap(
        meta.ptr(), (int)params.size(), meta.num_chunks,
        scalars.data_ptr<float>(), (int)group, (float)momentum,
        (float)dampening, (float)weight_decay, nesterov ? 1 : 0,
        current_stream(params[0]));
}

void fused_adam_cap(std::vector<torch::Tensor> params,
                    std::vector<torch::Tensor> grads,
                    std::vector<torch::Tensor> exp_avgs,
                    std::vector<torch::Tensor> exp_avg_sqs,
                    torch::Tensor scalars, int64_t group, double beta1,
                    double beta2, double eps, double weight_decay,
                    bool adamw) {
    Lists lists{params, grads, exp_avgs, exp_avg_sqs};
    check_lists(lists);
    check_scalars(scalars, group, params[0]);
    const auto& meta = get_meta(lists);
    swq_launch_fused_adam_cap(
        meta.ptr(), (int)params.size(), meta.num_chunks,
        scalars.data_ptr<float>(), (int)group, (float)beta1, (float)beta2,
        (float)eps, (float)weight_decay, adamw ? 1 : 0,
        current_stream(params[0]));
}

void clear_meta_cache() { g_meta_cache.clear(); }

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "shockwave_amd CDNA4 fused multi-tensor kernels";
    // the layout the kernels were compiled with; ops/__init__.py checks its
    // own copy against these at import
    m.attr("CHUNK_ELEMS") = CHUNK_ELEMS;
    m.attr("SCALAR_GRAD_NORM") = SWQ_SCALAR_GRAD_NORM;
    m.attr("SCALAR_CLIP_COEF") = SWQ_SCALAR_CLIP_COEF;
    m.attr("SCALAR_STEP") = SWQ_SCALAR_STEP;
    m.attr("SCALAR_LR0") = SWQ_SCALAR_LR0;
    m.def("fused_sgd", &fused_sgd, "fused multi-tensor SGD-momentum step");
    m.def("fused_adam", &fused_adam, "fused multi-tensor Adam/AdamW step");
    m.def("multi_tensor_accum", &multi_tensor_accum, "dst += alpha*src");
    m.def("multi_tensor_l2norm_sq", &multi_tensor_l2norm_sq,
          "per-tensor squared L2 norms");
    m.def("gns_window_stats", &gns_window_stats,
          "window-average + current grad squared norms");
    m.def("multi_tensor_sumsq_partials", &multi_tensor_sumsq_partials,
          "per-chunk sum of squares into partials[offset:]; returns chunks");
    m.def("optim_prologue", &optim_prologue,
          "global norm + clip coefficient + step advance (one block)");
    m.def("fused_sgd_cap", &fused_sgd_cap,
          "fused SGD step with device-side lr / step / clip");
    m.def("fused_adam_cap", &fused_adam_cap,
          "fused Adam/AdamW step with device-side lr / step / clip");
    m.def("clear_meta_cache", &clear_meta_cache);
}
