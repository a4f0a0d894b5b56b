// Host/kernel launch ABI of the spectral-norm kernels (_spectral extension).
// Included by spectral_norm.hip (definitions) and spectral_ext.cpp (calls).
//
// W is a row-major bf16 matrix [M, K]; u [M], v [K] and sig [2] = {sigma,
// 1 / max(sigma, eps)} are fp32 and live in device memory only.
#pragma once

#include <hip/hip_runtime.h>

extern "C" {

int sn_block_size();      // threads per block of every kernel
int sn_grid_cap();        // block cap of the grid-stride passes
int sn_chunk_rows();      // rows per column-pass chunk before the cap
int sn_max_chunks();      // cap on column-pass row chunks

// workspace sizes (fp32 elements) for a [M, K] matrix
long sn_chunks(long M);          // row chunks of the column pass
long sn_col_blocks(long K);      // norm partials of the column pass
long sn_dot_blocks(long M, long K);  // partials of the backward reduction

// One power iteration + W / sigma. u, v updated in place; u_out, v_out are
// the per-call copies; t [K] and s [M] are the unnormalised W^T u and W v.
void launch_sn_forward(const void* W, void* Wsn, float* u, float* v,
                       float* u_out, float* v_out, float* sig, float* tpart,
                       float* t, float* nsq_part, float* s, long M, long K,
                       hipStream_t st);

// sigma = u . (W v) from the stored vectors; writes s, sig and Wsn only.
void launch_sn_forward_eval(const void* W, void* Wsn, const float* u,
                            const float* v, float* sig, float* s, long M,
                            long K, hipStream_t st);

// dW = (G - <G, Wsn> u v^T) / sigma
void launch_sn_backward(const void* G, const void* Wsn, const float* u,
                        const float* v, const float* sig, float* dot_part,
                        void* dW, long M, long K, hipStream_t st);

}  // extern "C"
