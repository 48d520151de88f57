// What the LDPC feature kernels share (ldpc_datapath.hip; ldpc_code.hip): launch shape, the class pick, the normal draw and the gather
// stage behind the channel.
#pragma once
#include "fgnn_common.h"
#include <stdint.h>

#define LD_THREADS 256
#define LD_CW_PER_WG 64
#define LD_MAX_CHOICES 16

// choices[idx] without a dynamically indexed copy of the parameter block in scratch memory
__device__ __forceinline__ float ld_choice(const float (&choices)[LD_MAX_CHOICES], unsigned idx) {
    float v = choices[0];
#pragma unroll
    for (unsigned j = 1; j < LD_MAX_CHOICES; ++j) v = idx == j ? choices[j] : v;
    return v;
}

// standard normal from two 32-bit words (Box-Muller, cosine branch): u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ float ld_normal(unsigned a, unsigned b) {
    const float u1 = ((float)(a >> 8) + 1.0f) * 5.9604644775390625e-08f, u2 = (float)(b >> 8) * 5.9604644775390625e-08f;
    return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}


// The gather stage shared by both feature kernels: word b's received values ys [nvar] (in LDS) -> node [2][nvar] (ys, snr[n * snr_sn]),
// hop [dc][nchk], ef_f2v [dc+1][nvar][dv], ef_v2f [dc+1][nchk][dc], every output array written by flat index (coalesced).
template <typename T>
__device__ __forceinline__ void ld_gather_features(const float* ys, const float* snr, int64_t snr_sn, const int* var_to_factors,
                                                   const int* factor_to_vars, int64_t b, int nvar, int nchk, int dv, int dc, T* node_base,
                                                   T* hop_base, T* ef_f2v_base, T* ef_v2f_base) {
    const int tid = threadIdx.x;
    T* node = node_base + b * 2 * nvar;                                     // [2][nvar]
    for (int o = tid; o < 2 * nvar; o += LD_THREADS) fgnn_st(node + o, o < nvar ? ys[o] : snr[(o - nvar) * snr_sn]);
    T* hop = hop_base + b * dc * nchk;                                      // [dc][nchk] = hop^T
    for (int o = tid; o < dc * nchk; o += LD_THREADS) {
        const int j = o / nchk, f = o - j * nchk;
        fgnn_st(hop + o, ys[factor_to_vars[f * dc + j]]);
    }
    T* e1 = ef_f2v_base + b * (int64_t)(dc + 1) * nvar * dv;               // [dc+1][nvar][dv]
    for (int o = tid; o < (dc + 1) * nvar * dv; o += LD_THREADS) {
        const int c = o / (nvar * dv), r = o - c * nvar * dv, n = r / dv, j = r - n * dv;
        const float v = c < dc ? ys[factor_to_vars[var_to_factors[n * dv + j] * dc + c]] : ys[n];
        fgnn_st(e1 + o, v);
    }
    T* e2 = ef_v2f_base + b * (int64_t)(dc + 1) * nchk * dc;               // [dc+1][nchk][dc]
    for (int o = tid; o < (dc + 1) * nchk * dc; o += LD_THREADS) {
        const int c = o / (nchk * dc), r = o - c * nchk * dc, f = r / dc, j = r - f * dc;
        fgnn_st(e2 + o, ys[factor_to_vars[f * dc + (c < dc ? c : j)]]);
    }
}
