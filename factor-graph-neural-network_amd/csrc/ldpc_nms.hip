// ldpc_nms.hip — the learned ("neural") min-sum LDPC decoder: a flooding min-sum whose normalisation weights alpha and offsets beta
// are parameters per iteration, per (iteration, check) or per (iteration, edge), with the backward that trains them.  The reference has
// no counterpart; the steps are stated in include/fgnn_hip_ldpc_nms.h and restated in tests/ldpc_nms_oracle.py.
//
//   fgnn_ldpc_nms_forward                     one launch: decode mode (early stop) or train mode (every iteration's totals + the record)
//   fgnn_ldpc_nms_backward                    g_alpha, g_beta (batch sums, no floating-point atomics) and g_llr: two launches
//   fgnn_ldpc_nms_record_bytes, fgnn_ldpc_nms_backward_workspace_bytes, fgnn_ldpc_nms_lds_bytes, fgnn_ldpc_nms_backward_workgroups
//
// Built with -ffp-contract=off: the decode mode with constant weights is fgnn_ldpc_decode_llr's flooding min-sum bit for bit, and the
// backward recomputes u = alpha * mag - beta with the forward's own rounding.
//
// Forward layout: one workgroup per word, ldpc_word.h's state and thread rule; the min-sum scan, the variable pass and the violated-
// check count are its functions, the carve, staging and load rule are written out in the kernel.  The weights are read from global
// memory where they are used (one value per check update with share 0 / 1, one per edge with share 2).
//
// Record (train mode): ldpc_nms.h states it; a lane owns a check, so the planes are read and written coalesced.
//
// Backward layout: workgroup g of G = min(B, 512) takes the words g, g + G, ...; the same thread counts.  In LDS, ldpc_word.h's
// state with, in the places of R, T and prior, f32 gQ [E] (the g_q of the iteration above, by edge: variable n's edges are
// contiguous, so what an iteration sends back to T[n] is a gather in edge order, not a scatter), gT [N] (this iteration's total
// gradients) and gP [N] (g_prior), and 8 floats of wave sums as the scratch words; and the workgroup's partial of g_alpha / g_beta
// [2][n_iter W] where the whole stays within 64 KiB (two workgroups per CU and more), else in the workgroup's own slice of the
// workspace.  Every partial element has one owner thread (share 1: the check's lane; share 2: the edge's check's lane; share 0:
// thread 0, after a fixed-order wave and workgroup reduction), which adds to it word after word in the order of its words: no
// atomics, the same bits every time.  The second launch adds the G slices in a fixed order (ldpc_nms_sum_kernel).
#include "ldpc_nms.h"     // the limits, the parameters, nms_weight, the record, the argument checks: shared with ldpc_nms_layered.hip

// the state's bytes: 4 scratch ints forward, 8 floats backward
__host__ __device__ static inline int64_t nms_state_bytes(int N, int M, int E, int backward) {
    return ldpc_word_bytes_nms(N, M, E, backward ? 32 : 16);
}

template <bool TRAIN>
__global__ __launch_bounds__(256) void ldpc_nms_fwd_kernel(const NmsFwdParams p) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = p.N, M = p.M, E = p.E, share = p.share;
    const int W = share == 0 ? 1 : share == 1 ? M : E;
    const int64_t b = blockIdx.x;
    // ldpc_word_carve, ldpc_stage_tables and ldpc_load_word written out: as calls they cost the decode mode 1 %
    float* R = (float*)ldpc_lds;
    float* T = R + E;
    float* prior = T + N;
    uint32_t* rtab = (uint32_t*)(prior + N);
    int* wsum = (int*)(rtab + E);
    uint16_t* rp = (uint16_t*)(wsum + 4);
    uint16_t* cp = rp + (M + 1);
    const LdpcWord s = {R, T, prior, rtab, wsum, rp, cp};
    for (int e = tid; e < E; e += nt) {
        rtab[e] = ((uint32_t)p.row_edge[e] & 0xffffu) | ((uint32_t)p.row_var[e] << 16);
        R[e] = 0.0f;
    }
    for (int m = tid; m <= M; m += nt) rp[m] = (uint16_t)p.row_ptr[m];
    for (int n = tid; n <= N; n += nt) cp[n] = (uint16_t)p.col_ptr[n];
    const float* in = p.llr + b * p.llr_sb;
    for (int n = tid; n < N; n += nt) {
        float v = in[n];
        if (v != v) v = 0.0f;
        v = fminf(fmaxf(v, -LDPC_CLAMP), LDPC_CLAMP);
        prior[n] = v;
        T[n] = v;
    }
    __syncthreads();

    int it = 0, viol = 0;
    for (;;) {
        ++it;
        for (int m = tid; m < M; m += nt) {
            const int r0 = rp[m], r1 = rp[m + 1], L = r1 - r0;
            const LdpcMinScan c = ldpc_min_scan(s, r0, r1);
            if (TRAIN) {
                uint32_t* rec = p.record + NMS_RECORD_AT(b, p.n_iter, it, M, m);
                rec[0] = __float_as_uint(c.m1);
                rec[M] = __float_as_uint(c.m2);
                rec[2 * (int64_t)M] = nms_record_pack(c, r0);
            }
            float al = 0.0f, be = 0.0f;
            if (share != 2) { al = nms_weight(p.alpha, it, W, share, m, 0); be = nms_weight(p.beta, it, W, share, m, 0); }
            for (int r = r0; r < r1; ++r) {
                const int e = rtab[r] & 0xffffu;
                if (share == 2) { al = nms_weight(p.alpha, it, W, 2, m, e); be = nms_weight(p.beta, it, W, 2, m, e); }
                const float mag = r == c.i1 ? c.m2 : c.m1;
                const float u = al * mag - be;
                float o = fmaxf(u, 0.0f);
                if (c.par != (bool)((c.signs >> (r - r0)) & 1u)) o = -o;
                if (L == 1) o = 0.0f;
                R[e] = o;
            }
        }
        __syncthreads();
        for (int n = tid; n < N; n += nt) {
            const float sum = ldpc_var_sum(s, n, prior[n]);
            T[n] = sum;
            if (TRAIN) p.totals[((int64_t)(it - 1) * p.B + b) * N + n] = sum;
        }
        __syncthreads();
        viol = ldpc_count_violated(s, M);
        if ((!TRAIN && viol == 0) || it >= p.n_iter) break;
    }

    for (int n = tid; n < N; n += nt) {
        const float v = T[n];
        if (p.x) p.x[b * N + n] = v < 0.0f ? 1 : 0;
        if (p.post) p.post[b * N + n] = v;
    }
    if (tid == 0) {
        if (p.viol) p.viol[b] = viol;
        if (p.iters) p.iters[b] = it;
    }
}

// PART_LDS: the workgroup's partial [2][n_iter W] lies in LDS behind the state (and is copied to its workspace slice at the end);
// otherwise it is the slice itself.
template <bool PART_LDS>
__global__ __launch_bounds__(256) void ldpc_nms_bwd_kernel(const NmsBwdParams p) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int N = p.N, M = p.M, E = p.E, share = p.share, W = p.W, n_iter = p.n_iter;
    const int cnt = n_iter * W;
    const LdpcWord s = ldpc_word_carve(N, M, E, 8);
    float *gQ = s.R, *gT = s.T, *gP = s.prior, *red = (float*)s.wsum;
    const uint32_t* rtab = s.rtab;
    const uint16_t* rp = s.rp;
    float* slice = p.ws + (int64_t)blockIdx.x * 2 * cnt;
    float* part = PART_LDS ? (float*)(ldpc_lds + nms_state_bytes(N, M, E, 1)) : slice;

    ldpc_stage_tables(s, p, false);
    for (int i = tid; i < 2 * cnt; i += nt) part[i] = 0.0f;
    __syncthreads();

    for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
        for (int e = tid; e < E; e += nt) gQ[e] = 0.0f;
        for (int n = tid; n < N; n += nt) gP[n] = 0.0f;
        __syncthreads();
        for (int t = n_iter; t >= 1; --t) {
            for (int n = tid; n < N; n += nt) {                                 // gT_t = g_totals[t] + what iteration t + 1 sent back
                const float g = p.g_totals[((int64_t)(t - 1) * p.B + b) * N + n] + ldpc_var_sum(s, n, 0.0f);
                gT[n] = g;
                gP[n] += g;
            }
            __syncthreads();
            float sa = 0.0f, sb = 0.0f;                                         // share 0: this thread's part of the iteration's sums
            for (int m = tid; m < M; m += nt) {
                const int r0 = rp[m], L = rp[m + 1] - r0;
                const uint32_t* rec = p.record + NMS_RECORD_AT(b, n_iter, t, M, m);
                const float m1 = __uint_as_float(rec[0]), m2 = __uint_as_float(rec[M]);
                const uint32_t pk = rec[2 * (int64_t)M];
                const uint32_t signs = pk & 0xffffu;
                const int i1 = (pk >> 16) & 31u, i2 = (pk >> 21) & 31u;
                const bool par = __popc(signs) & 1;
                float al = 0.0f, be = 0.0f;
                if (share != 2) { al = nms_weight(p.alpha, t, W, share, m, 0); be = nms_weight(p.beta, t, W, share, m, 0); }
                float ca = 0.0f, cb = 0.0f, gm1 = 0.0f, gm2 = 0.0f;
                if (L > 1)
                    for (int l = 0; l < L; ++l) {
                        const uint32_t ev = rtab[r0 + l];
                        const int e = ev & 0xffffu;
                        if (share == 2) { al = nms_weight(p.alpha, t, W, 2, m, e); be = nms_weight(p.beta, t, W, 2, m, e); }
                        const float mag = l == i1 ? m2 : m1;
                        const float u = al * mag - be;
                        float go = gT[ev >> 16] - gQ[e];                        // g_e: gR_t[e] = -g_q_e of iteration t + 1
                        if (par != (bool)((signs >> l) & 1u)) go = -go;
                        if (!(u > 0.0f)) go = 0.0f;
                        const float ga = go * mag;
                        if (share == 2) {
                            float* pa = part + (int64_t)(t - 1) * W + e;
                            pa[0] += ga;
                            pa[cnt] -= go;
                        } else {
                            ca += ga;
                            cb -= go;
                        }
                        const float gmag = go * al;
                        if (l == i1) gm2 = gmag; else gm1 += gmag;
                    }
                for (int l = 0; l < L; ++l) {                                   // g_q: places i1 and i2 only
                    float gq = l == i1 ? gm1 : l == i2 ? gm2 : 0.0f;
                    if ((signs >> l) & 1u) gq = -gq;
                    gQ[rtab[r0 + l] & 0xffffu] = gq;
                }
                if (share == 1) {
                    float* pa = part + (int64_t)(t - 1) * W + m;
                    pa[0] += ca;
                    pa[cnt] += cb;
                } else {
                    sa += ca;
                    sb += cb;
                }
            }
            if (share == 0) {                                                   // lanes in a fixed order, then the waves in order
                for (int off = 32; off >= 1; off >>= 1) {
                    sa += __shfl_down(sa, off);
                    sb += __shfl_down(sb, off);
                }
                if (lane == 0) { red[2 * wave] = sa; red[2 * wave + 1] = sb; }
            }
            __syncthreads();
            if (share == 0 && tid == 0) {       // (red is written again only behind the next iteration's first barrier)
                float a = red[0], c = red[1];
                for (int w = 1; w < nw; ++w) { a += red[2 * w]; c += red[2 * w + 1]; }
                part[t - 1] += a;
                part[cnt + t - 1] += c;
            }
        }
        for (int n = tid; n < N; n += nt) {                                     // t = 0: T_0 = prior
            const float g = ldpc_var_sum(s, n, gP[n]);
            if (p.g_llr) {
                const float v = p.llr[b * p.llr_sb + n];
                p.g_llr[b * N + n] = (v >= -LDPC_CLAMP && v <= LDPC_CLAMP) ? g : 0.0f;
            }
        }
        __syncthreads();
    }
    if (PART_LDS)
        for (int i = tid; i < 2 * cnt; i += nt) slice[i] = part[i];
}

// out[i] = the sum over the slices g of ws[g][i], i over [2][cnt] (g_alpha then g_beta), in a fixed order: lane group k of 8 adds the
// slices g = k, k + 8, ... in that order, then one thread adds the 8 sums in the order k = 0 .. 7.  32 outputs per workgroup: a group
// reads 128 contiguous bytes of a slice.
__global__ __launch_bounds__(256) void ldpc_nms_sum_kernel(const float* ws, int G, int cnt, float* g_alpha, float* g_beta) {
    __shared__ float sh[8][32];
    const int ii = threadIdx.x & 31, k = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + ii;
    float s = 0.0f;
    if (i < 2 * cnt)
        for (int g = k; g < G; g += 8) s += ws[(int64_t)g * 2 * cnt + i];
    sh[k][ii] = s;
    __syncthreads();
    if (k != 0 || i >= 2 * cnt) return;
    for (int j = 1; j < 8; ++j) s += sh[j][ii];
    if (i < cnt) g_alpha[i] = s; else g_beta[i - cnt] = s;
}

extern "C" int64_t fgnn_ldpc_nms_lds_bytes(int N, int M, int E, int backward) {
    if (nms_check_sizes("ldpc_nms_lds_bytes", 0, N, M, E, 1, 0) != FGNN_OK) return -1;
    return nms_state_bytes(N, M, E, backward != 0);
}

extern "C" int64_t fgnn_ldpc_nms_record_bytes(int64_t B, int N, int M, int E, int n_iter) {
    if (nms_check_sizes("ldpc_nms_record_bytes", B, N, M, E, n_iter, 0) != FGNN_OK) return -1;
    return nms_record_bytes(B, M, n_iter);
}

extern "C" int64_t fgnn_ldpc_nms_backward_workgroups(int64_t B) { return nms_groups(B); }

extern "C" int64_t fgnn_ldpc_nms_backward_workspace_bytes(int64_t B, int N, int M, int E, int n_iter, int share) {
    if (nms_check_sizes("ldpc_nms_backward_workspace_bytes", B, N, M, E, n_iter, share) != FGNN_OK) return -1;
    const int64_t W = share == 0 ? 1 : share == 1 ? M : E;
    return nms_groups(B) * 2 * n_iter * W * 4;
}

extern "C" int fgnn_ldpc_nms_forward(const float* llr, int64_t llr_sb, const int32_t* col_ptr, const int32_t* row_ptr,
                                     const int32_t* row_edge, const int32_t* row_var, const float* alpha, const float* beta, int64_t B,
                                     int N, int M, int E, int n_iter, int share, int stop_early, uint8_t* x, float* post, int32_t* viol,
                                     int32_t* iters, float* totals, void* record, int64_t record_bytes, fgnn_stream_t stream) {
    NmsFwdParams p = {};
    if (int rc = nms_forward_args("ldpc_nms_forward", llr, llr_sb, col_ptr, row_ptr, row_edge, row_var, alpha, beta, B, N, M, E, n_iter,
                                  share, stop_early, x, post, viol, iters, totals, record, record_bytes, &p))
        return rc;
    if (B == 0) return FGNN_OK;
    void (*kernel)(const NmsFwdParams) = stop_early ? ldpc_nms_fwd_kernel<false> : ldpc_nms_fwd_kernel<true>;
    const int threads = ldpc_word_threads(N, M), lds = (int)nms_state_bytes(N, M, E, 0);
    fgnn_note_kernel("ldpc_nms_fwd_kernel<%d>x%d", !stop_early, threads);
    return fgnn_launch("ldpc_nms_forward", kernel, dim3((unsigned)B), dim3(threads), lds, fgnn_stream(stream), p);
}

int nms_launch_sum(const char* what, const float* ws, int G, int cnt, float* g_alpha, float* g_beta, hipStream_t st) {
    return fgnn_launch(what, ldpc_nms_sum_kernel, dim3((unsigned)((2 * cnt + 31) / 32)), dim3(256), 0, st, ws, G, cnt, g_alpha, g_beta);
}

extern "C" int fgnn_ldpc_nms_backward(const float* g_totals, const float* llr, int64_t llr_sb, const int32_t* col_ptr,
                                      const int32_t* row_ptr, const int32_t* row_edge, const int32_t* row_var, const float* alpha,
                                      const float* beta, const void* record, int64_t record_bytes, int64_t B, int N, int M, int E,
                                      int n_iter, int share, float* g_alpha, float* g_beta, float* g_llr, void* workspace,
                                      int64_t workspace_bytes, fgnn_stream_t stream) {
    NmsBwdParams p = {};
    if (int rc = nms_backward_args("ldpc_nms_backward", g_totals, llr, llr_sb, col_ptr, row_ptr, row_edge, row_var, alpha, beta, record,
                                   record_bytes, B, N, M, E, n_iter, share, g_alpha, g_beta, g_llr, workspace, workspace_bytes, &p))
        return rc;
    const int cnt = n_iter * p.W;
    if (B == 0) return nms_backward_empty("ldpc_nms_backward", g_alpha, g_beta, cnt, fgnn_stream(stream));
    const int G = (int)nms_groups(B);
    const int64_t state = nms_state_bytes(N, M, E, 1);
    const bool part_lds = state + 8 * (int64_t)cnt <= NMS_PARTIAL_LDS;
    void (*kernel)(const NmsBwdParams) = part_lds ? ldpc_nms_bwd_kernel<true> : ldpc_nms_bwd_kernel<false>;
    const int threads = ldpc_word_threads(N, M), lds = (int)(state + (part_lds ? 8 * (int64_t)cnt : 0));
    fgnn_note_kernel("ldpc_nms_bwd_kernel<%d>x%d", part_lds, threads);
    if (int rc = fgnn_launch("ldpc_nms_backward", kernel, dim3((unsigned)G), dim3(threads), lds, fgnn_stream(stream), p)) return rc;
    return nms_launch_sum("ldpc_nms_backward sum", (const float*)workspace, G, cnt, g_alpha, g_beta, fgnn_stream(stream));
}
