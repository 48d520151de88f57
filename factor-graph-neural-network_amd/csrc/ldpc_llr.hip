// ldpc_llr.hip — LLR-domain LDPC decoders for a batch of received words: normalized min-sum, offset min-sum and sum-product, each
// with a flooding or a layered schedule.  The reference has no counterpart (its one classical decoder is ldpc_decode.hip's); the
// steps are derived here and restated in tests/ldpc_llr_oracle.py.
//
//   fgnn_ldpc_decode_llr              one launch decodes the batch: hard decisions, totals, violated checks, iterations
//   fgnn_ldpc_decode_llr_lds_bytes    the LDS one word occupies, or < 0 where the shape is not taken
//
// The tables, the per-word LDS layout, the thread rule and the steps shared with the learned min-sum kernels (staging, load, variable
// pass, violated-check count, the min-sum scan) are ldpc_word.h's.  Layers: the checks of layer k are layer_chk[layer_ptr[k] ..
// layer_ptr[k + 1] - 1]; no two of them share a variable.
//
// Steps, all f32, each expression in the order written (this file is built with -ffp-contract=off):
//   load     prior[n] = llr[n]; NaN -> 0; clamped to +-4096.  T[n] = prior[n], R[e] = 0.
//   check m  over its edges l = 0 .. L-1:  q_l = T[var_l] - R[edge_l]; q_l counts as negative exactly when q_l < 0.
//            0  R'_l = s_l (alpha * min_{k != l} |q_k|)              s_l = -1 when an odd number of the OTHER q are negative, else +1
//            1  R'_l = s_l max(min_{k != l} |q_k| - beta, 0)
//            2  t_l = tanhf(0.5f q_l); F_0 = 1, F_{l+1} = F_l t_l; S_L = 1, S_l = S_{l+1} t_l; p_l = F_l S_{l+1} clamped to
//               +-(1 - 2^-24); R'_l = 2 atanhf(p_l)
//            L = 1: R'_0 = 0.
//   flooding iteration   every check from the old T, R[edge_l] = R'_l; then T[n] = prior[n] + R[col_ptr[n]] + R[col_ptr[n] + 1] + ...
//   layered iteration    the layers in order, a barrier after each; a check stores R[edge_l] = R'_l and T[var_l] = q_l + R'_l.
//   after an iteration   viol = the number of checks with an odd number of T[var] < 0; stop when viol = 0 or at max_iter.
//   outputs  x[n] = T[n] < 0, post[n] = T[n], viol, iters (>= 1).
//   overflow min-sum messages that feed back (a dense code under the layered schedule) can carry T past the f32 range: infinities follow
//            IEEE; a NaN q (inf - inf) is skipped by the two minima (both comparisons are `<`), counts as non-negative and makes the
//            totals it enters NaN, whose hard decision is 0.  Sum-product messages are at most 2 atanhf(1 - 2^-24) = 17.33: no overflow.
//
// Layout: one workgroup per word, ldpc_word.h's state for the whole run with 16-bit layer_chk [M], layer_ptr [M + 1] appended.  Global
// memory is read once (tables, llr) and written once.  A lane runs one check's update at a time: min-sum in two sweeps over the
// check's edges (ldpc_min_scan, then the emit: no array), sum-product with its 16 tanh values and prefix products in registers
// (fully unrolled, predicated on L).
#include "fgnn_hip_ldpc_llr.h"
#include "ldpc_word.h"

#define LLR_PMAX 0.99999994f        // 1 - 2^-24

struct LlrParams {
    const float* llr; int64_t llr_sb;
    const int32_t *col_ptr, *row_ptr, *row_edge, *row_var, *layer_ptr, *layer_chk;
    uint8_t* x;
    float* post;
    int32_t *viol, *iters;
    int N, M, E, n_layers, max_iter;
    float alpha, beta;
};

struct LlrLds : LdpcWord { uint16_t *lc, *lp; };        // the layer tables, behind cp

__device__ __forceinline__ LlrLds llr_carve(int N, int M, int E) {
    LlrLds s;
    (LdpcWord&)s = ldpc_word_carve(N, M, E, 4);
    s.lc = s.cp + (N + 1);
    s.lp = s.lc + M;
    return s;
}

// one check's update (see Steps)
template <int ALG, bool LAYERED>
__device__ __forceinline__ void llr_check(const LdpcWord& s, int m, float alpha, float beta) {
    const int r0 = s.rp[m], r1 = s.rp[m + 1], L = r1 - r0;
    if (ALG != 2) {
        const LdpcMinScan c = ldpc_min_scan(s, r0, r1);
        for (int r = r0; r < r1; ++r) {
            const uint32_t ev = s.rtab[r];
            const int e = ev & 0xffffu, v = ev >> 16;
            const float q = s.T[v] - s.R[e];
            const float mag = r == c.i1 ? c.m2 : c.m1;
            float o = ALG == 0 ? alpha * mag : fmaxf(mag - beta, 0.0f);
            if (c.par != (q < 0.0f)) o = -o;
            if (L == 1) o = 0.0f;
            s.R[e] = o;
            if (LAYERED) s.T[v] = q + o;
        }
    } else {
        float t[LDPC_MAXD], pf[LDPC_MAXD];
        float F = 1.0f;
#pragma unroll
        for (int l = 0; l < LDPC_MAXD; ++l)
            if (l < L) {
                const uint32_t ev = s.rtab[r0 + l];
                const float q = s.T[ev >> 16] - s.R[ev & 0xffffu];
                t[l] = tanhf(0.5f * q);
                pf[l] = F;
                F = F * t[l];
            }
        float S = 1.0f;
#pragma unroll
        for (int l = LDPC_MAXD - 1; l >= 0; --l)
            if (l < L) {
                const uint32_t ev = s.rtab[r0 + l];
                const int e = ev & 0xffffu, v = ev >> 16;
                const float q = s.T[v] - s.R[e];
                float pl = pf[l] * S;
                S = S * t[l];
                pl = fminf(fmaxf(pl, -LLR_PMAX), LLR_PMAX);
                float o = 2.0f * atanhf(pl);
                if (L == 1) o = 0.0f;
                s.R[e] = o;
                if (LAYERED) s.T[v] = q + o;
            }
    }
}

template <int ALG, bool LAYERED>
__global__ __launch_bounds__(256) void ldpc_llr_kernel(const LlrParams p) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = p.N, M = p.M;
    const int64_t b = blockIdx.x;
    const LlrLds s = llr_carve(N, M, p.E);

    ldpc_stage_tables(s, p, true);
    if (LAYERED) {
        for (int i = tid; i < M; i += nt) s.lc[i] = (uint16_t)p.layer_chk[i];
        for (int k = tid; k <= p.n_layers; k += nt) s.lp[k] = (uint16_t)p.layer_ptr[k];
    }
    ldpc_load_word(s, p.llr + b * p.llr_sb, N);
    __syncthreads();

    const float alpha = p.alpha, beta = p.beta;
    int it = 0, viol = 0;
    for (;;) {
        ++it;
        if (!LAYERED) {
            for (int m = tid; m < M; m += nt) llr_check<ALG, false>(s, m, alpha, beta);
            __syncthreads();
            for (int n = tid; n < N; n += nt) s.T[n] = ldpc_var_sum(s, n, s.prior[n]);
            __syncthreads();
        } else {
            for (int k = 0; k < p.n_layers; ++k) {
                const int i1 = s.lp[k + 1];
                for (int i = s.lp[k] + tid; i < i1; i += nt) llr_check<ALG, true>(s, s.lc[i], alpha, beta);
                __syncthreads();
            }
        }
        viol = ldpc_count_violated(s, M);
        if (viol == 0 || it >= p.max_iter) break;
    }

    for (int n = tid; n < N; n += nt) {
        const float v = s.T[n];
        p.x[b * N + n] = v < 0.0f ? 1 : 0;
        if (p.post) p.post[b * N + n] = v;
    }
    if (tid == 0) { p.viol[b] = viol; p.iters[b] = it; }
}

extern "C" int64_t fgnn_ldpc_decode_llr_lds_bytes(int N, int M, int E) {
    return ldpc_word_check_sizes("ldpc_decode_llr", N, M, E) == FGNN_OK ? ldpc_word_bytes_llr(N, M, E) : -1;
}

typedef void (*llr_kernel_t)(const LlrParams);

extern "C" int fgnn_ldpc_decode_llr(const float* llr, int64_t llr_sb, const int32_t* col_ptr, const int32_t* row_ptr,
                                    const int32_t* row_edge, const int32_t* row_var, const int32_t* layer_ptr,
                                    const int32_t* layer_chk, int n_layers, int64_t B, int N, int M, int E, int algorithm,
                                    int max_iter, float alpha, float beta, uint8_t* x, float* post, int32_t* viol, int32_t* iters,
                                    fgnn_stream_t stream) {
    const int64_t per = fgnn_ldpc_decode_llr_lds_bytes(N, M, E);
    if (per < 0) return FGNN_EUNSUPPORTED;
    if (algorithm < 0 || algorithm > 2) FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_decode_llr: algorithm=%d outside 0..2", algorithm);
    if (B < 0 || B > 0x7fffffffll) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_llr: batch %lld outside 0 .. 2^31-1", (long long)B);
    if (max_iter < 1) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_llr: max_iter=%d is below 1", max_iter);
    if (!(alpha >= 0.0f && alpha <= 3.0e38f)) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_llr: alpha=%g is not a finite value >= 0", alpha);
    if (!(beta >= 0.0f && beta <= 3.0e38f)) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_llr: beta=%g is not a finite value >= 0", beta);
    if (llr_sb < 0) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_llr: negative row stride");
    if (n_layers < 0 || n_layers > M) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_llr: n_layers=%d outside 0..M=%d", n_layers, M);
    if (B == 0) return FGNN_OK;
    if (!llr || !col_ptr || !row_ptr || !row_edge || !row_var) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_llr: null input pointer");
    if (n_layers > 0 && (!layer_ptr || !layer_chk)) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_llr: null layer table with n_layers=%d", n_layers);
    if (!x || !viol || !iters) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_llr: null output pointer");
    LlrParams p = {};
    p.llr = llr; p.llr_sb = llr_sb;
    p.col_ptr = col_ptr; p.row_ptr = row_ptr; p.row_edge = row_edge; p.row_var = row_var;
    p.layer_ptr = layer_ptr; p.layer_chk = layer_chk;
    p.x = x; p.post = post; p.viol = viol; p.iters = iters;
    p.N = N; p.M = M; p.E = E; p.n_layers = n_layers; p.max_iter = max_iter;
    p.alpha = alpha; p.beta = beta;
    static const llr_kernel_t kernels[3][2] = {{ldpc_llr_kernel<0, false>, ldpc_llr_kernel<0, true>},
                                               {ldpc_llr_kernel<1, false>, ldpc_llr_kernel<1, true>},
                                               {ldpc_llr_kernel<2, false>, ldpc_llr_kernel<2, true>}};
    const llr_kernel_t kernel = kernels[algorithm][n_layers > 0];
    const int threads = ldpc_word_threads(N, M), lds = (int)per;
    fgnn_note_kernel("ldpc_llr_kernel<%d,%d>x%d", algorithm, n_layers > 0, threads);
    return fgnn_launch("ldpc_decode_llr", kernel, dim3((unsigned)B), dim3(threads), lds, fgnn_stream(stream), p);
}
