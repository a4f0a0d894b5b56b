// Torch bindings of the spectral-norm kernels (_spectral extension).
// A second module, so the frozen surface of _C stays what it is.  Thin
// layer: checks, allocation, stream plumbing; compute is in
// spectral_norm.hip, reached through spectral_abi.h.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "spectral_abi.h"

namespace {

hipStream_t cur_stream() {
  return (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
}

// W (or a gradient of it): bf16, contiguous, at least 1-D; viewed [M, K]
// with M = size(0)
void check_matrix(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() >= 1 && t.numel() > 0, name, " must not be empty");
}

void check_vec(const torch::Tensor& t, const torch::Tensor& w, int64_t n,
               const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == w.device(), name,
              " must be on the same device as w");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.numel() == n, name, " must have ", n, " elements, got ",
              t.numel());
}

torch::Tensor f32_buf(const torch::Tensor& like, int64_t n) {
  return torch::empty({n}, like.options().dtype(torch::kFloat32));
}

// (w_sn, u_copy, v_copy, sig[2] = {sigma, 1/max(sigma, eps)}, t, s);
// u and v are updated in place
std::vector<torch::Tensor> sn_forward(torch::Tensor w, torch::Tensor u,
                                      torch::Tensor v) {
  check_matrix(w, "w");
  int64_t M = w.size(0), K = w.numel() / M;
  check_vec(u, w, M, "u");
  check_vec(v, w, K, "v");
  torch::Tensor w_sn = torch::empty_like(w);
  torch::Tensor u_out = torch::empty_like(u), v_out = torch::empty_like(v);
  torch::Tensor sig = f32_buf(u, 2), t = f32_buf(u, K), s = f32_buf(u, M);
  torch::Tensor tpart = f32_buf(u, sn_chunks(M) * K);
  torch::Tensor nsq = f32_buf(u, sn_col_blocks(K));
  launch_sn_forward(w.data_ptr(), w_sn.data_ptr(), u.data_ptr<float>(),
                    v.data_ptr<float>(), u_out.data_ptr<float>(),
                    v_out.data_ptr<float>(), sig.data_ptr<float>(),
                    tpart.data_ptr<float>(), t.data_ptr<float>(),
                    nsq.data_ptr<float>(), s.data_ptr<float>(), (long)M,
                    (long)K, cur_stream());
  return {w_sn, u_out, v_out, sig, t, s};
}

// (w_sn, sig, s); u and v are only read
std::vector<torch::Tensor> sn_forward_eval(torch::Tensor w, torch::Tensor u,
                                           torch::Tensor v) {
  check_matrix(w, "w");
  int64_t M = w.size(0), K = w.numel() / M;
  check_vec(u, w, M, "u");
  check_vec(v, w, K, "v");
  torch::Tensor w_sn = torch::empty_like(w);
  torch::Tensor sig = f32_buf(u, 2), s = f32_buf(u, M);
  launch_sn_forward_eval(w.data_ptr(), w_sn.data_ptr(), u.data_ptr<float>(),
                         v.data_ptr<float>(), sig.data_ptr<float>(),
                         s.data_ptr<float>(), (long)M, (long)K, cur_stream());
  return {w_sn, sig, s};
}

// (dW, dot_part): dW = (g - <g, w_sn> u v^T) / sigma
std::vector<torch::Tensor> sn_backward(torch::Tensor g, torch::Tensor w_sn,
                                       torch::Tensor u, torch::Tensor v,
                                       torch::Tensor sig) {
  check_matrix(g, "g");
  check_matrix(w_sn, "w_sn");
  TORCH_CHECK(g.sizes() == w_sn.sizes() && g.device() == w_sn.device(),
              "g and w_sn must have the same shape and device");
  int64_t M = g.size(0), K = g.numel() / M;
  check_vec(u, g, M, "u");
  check_vec(v, g, K, "v");
  check_vec(sig, g, 2, "sig");
  torch::Tensor dw = torch::empty_like(g);
  torch::Tensor part = f32_buf(u, sn_dot_blocks(M, K));
  launch_sn_backward(g.data_ptr(), w_sn.data_ptr(), u.data_ptr<float>(),
                     v.data_ptr<float>(), sig.data_ptr<float>(),
                     part.data_ptr<float>(), dw.data_ptr(), (long)M, (long)K,
                     cur_stream());
  return {dw, part};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("sn_forward", &sn_forward,
          "power iteration + W / sigma; u, v updated in place on device");
  mod.def("sn_forward_eval", &sn_forward_eval,
          "W / (u . W v) from the stored vectors; writes no state");
  mod.def("sn_backward", &sn_backward,
          "dW = (g - <g, w_sn> u v^T) / sigma");
  mod.attr("SN_BLOCK") = sn_block_size();
  mod.attr("SN_GRID_CAP") = sn_grid_cap();
  mod.attr("SN_CHUNK_ROWS") = sn_chunk_rows();
  mod.attr("SN_MAX_CHUNKS") = sn_max_chunks();
}
