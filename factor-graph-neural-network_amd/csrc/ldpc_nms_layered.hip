// ldpc_nms_layered.hip — the learned min-sum LDPC decoder with a layered schedule: ldpc_nms.hip's decoder with the checks taken layer
// by layer, every check reading the totals the earlier layers of the same iteration left.  The reference has no counterpart; the
// steps are stated in include/fgnn_hip_ldpc_nms_layered.h and restated in tests/ldpc_nms_layered_oracle.py.
//
//   fgnn_ldpc_nms_layered_forward             one launch: decode mode (early stop) or train mode (every iteration's totals + the record)
//   fgnn_ldpc_nms_layered_backward            g_alpha, g_beta (batch sums, no floating-point atomics) and g_llr: two launches
//   fgnn_ldpc_nms_layered_lds_bytes
//
// Built with -ffp-contract=off: the decode mode with constant weights is fgnn_ldpc_decode_llr's layered min-sum bit for bit, and the
// backward recomputes u = alpha * mag - beta with the forward's own rounding.  The limits, the parameters, the weight index, the
// record and the argument checks are ldpc_nms.h's; the record's and the workspace's sizes are ldpc_nms.hip's queries.
//
// Forward layout: one workgroup per word, ldpc_word.h's state and thread rule with 16-bit layer_chk [M], layer_ptr [M + 1] appended
// (as ldpc_llr.hip).  Per layer a thread-strided loop over the layer's checks, then one barrier; a lane runs a whole check: the scan,
// the record, then the edge loop that stores R and T.  Inside a layer consecutive lanes hold the checks layer_chk names, so the
// record's planes are written coalesced only as far as those are consecutive.  n_layers + 1 barriers per iteration (the last is the
// violated-check count's).
//
// Backward layout: workgroup g of G = min(B, 512) takes the words g, g + G, ...; the same thread counts.  In LDS f32 gR [E], gT [N],
// the packed row table [E], 8 floats of wave sums, 16-bit row_ptr, layer_chk, layer_ptr (neither prior nor col_ptr: T' = q + R' sends
// the gradient of a total straight to q, there is no variable pass), and the workgroup's partial of g_alpha / g_beta [2][n_iter W]
// where the whole stays within 64 KiB, else in the workgroup's own slice of the workspace.  Ownership of the partial as in
// ldpc_nms.hip: share 2 the edge's check's lane, share 1 the check's lane (a check has the same place in its layer for every word, so
// the same lane), share 0 thread 0 after each thread has summed its checks of all layers of the iteration in registers and one
// fixed-order wave and workgroup reduction per iteration.  n_layers + 1 barriers per iteration, one more with share 0.
#include "fgnn_hip_ldpc_nms_layered.h"
#include "ldpc_nms.h"

struct NmsLayers { const int32_t *layer_ptr, *layer_chk; int n_layers; };
struct NmsLayeredFwdParams : NmsFwdParams { NmsLayers layers; };
struct NmsLayeredBwdParams : NmsBwdParams { NmsLayers layers; };

__host__ __device__ static inline int64_t nms_r16(int64_t v) { return (v + 15) / 16 * 16; }

// the state's bytes (the header's formula)
__host__ __device__ static inline int64_t nms_layered_state_bytes(int N, int M, int E, int backward) {
    if (backward) return nms_r16(4 * (2 * (int64_t)E + N) + 32) + nms_r16(2 * ((int64_t)(M + 1) + M + (M + 1)));
    return nms_r16(4 * (2 * (int64_t)E + 2 * (int64_t)N) + 16) + nms_r16(2 * ((int64_t)(M + 1) + (N + 1) + M + (M + 1)));
}

// the layer tables into LDS: lc [M], lp [n_layers + 1]
__device__ __forceinline__ void nms_stage_layers(uint16_t* lc, uint16_t* lp, const NmsLayers& y, int M) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < M; i += nt) lc[i] = (uint16_t)y.layer_chk[i];
    for (int k = tid; k <= y.n_layers; k += nt) lp[k] = (uint16_t)y.layer_ptr[k];
}

template <bool TRAIN>
__global__ __launch_bounds__(256) void ldpc_nms_layered_fwd_kernel(const NmsLayeredFwdParams p) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = p.N, M = p.M, E = p.E, share = p.share, n_layers = p.layers.n_layers;
    const int W = share == 0 ? 1 : share == 1 ? M : E;
    const int64_t b = blockIdx.x;
    const LdpcWord s = ldpc_word_carve(N, M, E, 4);
    float *R = s.R, *T = s.T;
    const uint32_t* rtab = s.rtab;
    const uint16_t* rp = s.rp;
    uint16_t* lc = s.cp + (N + 1);
    uint16_t* lp = lc + M;

    ldpc_stage_tables(s, p, true);
    nms_stage_layers(lc, lp, p.layers, M);
    ldpc_load_word(s, p.llr + b * p.llr_sb, N);
    __syncthreads();

    int it = 0, viol = 0;
    for (;;) {
        ++it;
        for (int k = 0; k < n_layers; ++k) {
            const int iend = lp[k + 1];
            for (int i = lp[k] + tid; i < iend; i += nt) {
                const int m = lc[i];
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
                    const uint32_t ev = rtab[r];
                    const int e = ev & 0xffffu, v = ev >> 16;
                    if (share == 2) { al = nms_weight(p.alpha, it, W, 2, m, e); be = nms_weight(p.beta, it, W, 2, m, e); }
                    const float q = T[v] - R[e];
                    const float mag = r == c.i1 ? c.m2 : c.m1;
                    const float u = al * mag - be;
                    float o = fmaxf(u, 0.0f);
                    if (c.par != (q < 0.0f)) o = -o;
                    if (L == 1) o = 0.0f;
                    R[e] = o;
                    T[v] = q + o;
                }
            }
            __syncthreads();
        }
        if (TRAIN)                          // T rests until the next iteration's first layer, behind the count's barrier
            for (int n = tid; n < N; n += nt) p.totals[((int64_t)(it - 1) * p.B + b) * N + n] = T[n];
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
__global__ __launch_bounds__(256) void ldpc_nms_layered_bwd_kernel(const NmsLayeredBwdParams p) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int N = p.N, M = p.M, E = p.E, share = p.share, W = p.W, n_iter = p.n_iter, n_layers = p.layers.n_layers;
    const int cnt = n_iter * W;
    float* gR = (float*)ldpc_lds;
    float* gT = gR + E;
    uint32_t* rtab = (uint32_t*)(gT + N);
    float* red = (float*)(rtab + E);
    uint16_t* rp = (uint16_t*)(red + 8);
    uint16_t* lc = rp + (M + 1);
    uint16_t* lp = lc + M;
    float* slice = p.ws + (int64_t)blockIdx.x * 2 * cnt;
    float* part = PART_LDS ? (float*)(ldpc_lds + nms_layered_state_bytes(N, M, E, 1)) : slice;

    for (int e = tid; e < E; e += nt) rtab[e] = ((uint32_t)p.row_edge[e] & 0xffffu) | ((uint32_t)p.row_var[e] << 16);
    for (int m = tid; m <= M; m += nt) rp[m] = (uint16_t)p.row_ptr[m];
    nms_stage_layers(lc, lp, p.layers, M);
    for (int i = tid; i < 2 * cnt; i += nt) part[i] = 0.0f;
    __syncthreads();

    for (int64_t b = blockIdx.x; b < p.B; b += gridDim.x) {
        for (int e = tid; e < E; e += nt) gR[e] = 0.0f;     // (behind the barrier of the word before's last layer)
        for (int n = tid; n < N; n += nt) gT[n] = 0.0f;     // (thread tid read gT[n] for g_llr itself)
        for (int t = n_iter; t >= 1; --t) {
            for (int n = tid; n < N; n += nt) gT[n] += p.g_totals[((int64_t)(t - 1) * p.B + b) * N + n];
            __syncthreads();
            float sa = 0.0f, sb = 0.0f;                     // share 0: this thread's part of the iteration's sums
            for (int k = n_layers - 1; k >= 0; --k) {
                const int iend = lp[k + 1];
                for (int i = lp[k] + tid; i < iend; i += nt) {
                    const int m = lc[i];
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
                            float go = gT[ev >> 16] + gR[e];                    // g_e
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
                    for (int l = 0; l < L; ++l) {                               // g_q = gT + the scan's part (places i1 and i2 only)
                        const uint32_t ev = rtab[r0 + l];
                        float gs = l == i1 ? gm1 : l == i2 ? gm2 : 0.0f;
                        if ((signs >> l) & 1u) gs = -gs;
                        const float gq = gT[ev >> 16] + gs;
                        gT[ev >> 16] = gq;
                        gR[ev & 0xffffu] = -gq;
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
                __syncthreads();
            }
            if (share == 0) {                               // lanes in a fixed order, then the waves in order; once per iteration
                for (int off = 32; off >= 1; off >>= 1) {
                    sa += __shfl_down(sa, off);
                    sb += __shfl_down(sb, off);
                }
                if (lane == 0) { red[2 * wave] = sa; red[2 * wave + 1] = sb; }
                __syncthreads();
                if (tid == 0) {                             // (red is written again only behind the next iteration's barriers)
                    float a = red[0], c = red[1];
                    for (int w = 1; w < nw; ++w) { a += red[2 * w]; c += red[2 * w + 1]; }
                    part[t - 1] += a;
                    part[cnt + t - 1] += c;
                }
            }
        }
        if (p.g_llr)
            for (int n = tid; n < N; n += nt) {
                const float v = p.llr[b * p.llr_sb + n];
                p.g_llr[b * N + n] = (v >= -LDPC_CLAMP && v <= LDPC_CLAMP) ? gT[n] : 0.0f;
            }
    }
    if (PART_LDS) {
        __syncthreads();
        for (int i = tid; i < 2 * cnt; i += nt) slice[i] = part[i];
    }
}

extern "C" int64_t fgnn_ldpc_nms_layered_lds_bytes(int N, int M, int E, int backward) {
    if (nms_check_sizes("ldpc_nms_layered_lds_bytes", 0, N, M, E, 1, 0) != FGNN_OK) return -1;
    return nms_layered_state_bytes(N, M, E, backward != 0);
}

extern "C" int fgnn_ldpc_nms_layered_forward(const float* llr, int64_t llr_sb, const int32_t* col_ptr, const int32_t* row_ptr,
                                             const int32_t* row_edge, const int32_t* row_var, const int32_t* layer_ptr,
                                             const int32_t* layer_chk, int n_layers, const float* alpha, const float* beta, int64_t B,
                                             int N, int M, int E, int n_iter, int share, int stop_early, uint8_t* x, float* post,
                                             int32_t* viol, int32_t* iters, float* totals, void* record, int64_t record_bytes,
                                             fgnn_stream_t stream) {
    const char* who = "ldpc_nms_layered_forward";
    NmsLayeredFwdParams p = {};
    if (int rc = nms_forward_args(who, llr, llr_sb, col_ptr, row_ptr, row_edge, row_var, alpha, beta, B, N, M, E, n_iter, share,
                                  stop_early, x, post, viol, iters, totals, record, record_bytes, &p))
        return rc;
    if (int rc = nms_check_layers(who, layer_ptr, layer_chk, n_layers, M, B)) return rc;
    if (B == 0) return FGNN_OK;
    p.layers = {layer_ptr, layer_chk, n_layers};
    void (*kernel)(const NmsLayeredFwdParams) = stop_early ? ldpc_nms_layered_fwd_kernel<false> : ldpc_nms_layered_fwd_kernel<true>;
    const int threads = ldpc_word_threads(N, M), lds = (int)nms_layered_state_bytes(N, M, E, 0);
    fgnn_note_kernel("ldpc_nms_layered_fwd_kernel<%d>x%d", !stop_early, threads);
    return fgnn_launch(who, kernel, dim3((unsigned)B), dim3(threads), lds, fgnn_stream(stream), p);
}

extern "C" int fgnn_ldpc_nms_layered_backward(const float* g_totals, const float* llr, int64_t llr_sb, const int32_t* col_ptr,
                                              const int32_t* row_ptr, const int32_t* row_edge, const int32_t* row_var,
                                              const int32_t* layer_ptr, const int32_t* layer_chk, int n_layers, const float* alpha,
                                              const float* beta, const void* record, int64_t record_bytes, int64_t B, int N, int M,
                                              int E, int n_iter, int share, float* g_alpha, float* g_beta, float* g_llr,
                                              void* workspace, int64_t workspace_bytes, fgnn_stream_t stream) {
    const char* who = "ldpc_nms_layered_backward";
    NmsLayeredBwdParams p = {};
    if (int rc = nms_backward_args(who, g_totals, llr, llr_sb, col_ptr, row_ptr, row_edge, row_var, alpha, beta, record, record_bytes, B,
                                   N, M, E, n_iter, share, g_alpha, g_beta, g_llr, workspace, workspace_bytes, &p))
        return rc;
    if (int rc = nms_check_layers(who, layer_ptr, layer_chk, n_layers, M, B)) return rc;
    const int cnt = n_iter * p.W;
    if (B == 0) return nms_backward_empty(who, g_alpha, g_beta, cnt, fgnn_stream(stream));
    p.layers = {layer_ptr, layer_chk, n_layers};
    const int G = (int)nms_groups(B);
    const int64_t state = nms_layered_state_bytes(N, M, E, 1);
    const bool part_lds = state + 8 * (int64_t)cnt <= NMS_PARTIAL_LDS;
    void (*kernel)(const NmsLayeredBwdParams) = part_lds ? ldpc_nms_layered_bwd_kernel<true> : ldpc_nms_layered_bwd_kernel<false>;
    const int threads = ldpc_word_threads(N, M), lds = (int)(state + (part_lds ? 8 * (int64_t)cnt : 0));
    fgnn_note_kernel("ldpc_nms_layered_bwd_kernel<%d>x%d", part_lds, threads);
    if (int rc = fgnn_launch(who, kernel, dim3((unsigned)G), dim3(threads), lds, fgnn_stream(stream), p)) return rc;
    return nms_launch_sum("ldpc_nms_layered_backward sum", (const float*)workspace, G, cnt, g_alpha, g_beta, fgnn_stream(stream));
}
