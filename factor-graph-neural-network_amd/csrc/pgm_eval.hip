// pgm_eval.hip — scores of decisions on the synthetic-PGM chain models, one launch per batch:
//
//   correct[b]     variables where the decision equals the label (the acc / acc_lp of train_syn_*.py's test loops,
//                  /root/reference/train_syn_hop_factor.py:349-409, train_syn_pw_factor.py:349-411, train_syn_fixed_pw_hop.py:313-362)
//   nll[b]         sum over the variables of F.cross_entropy's summand, logsumexp(v0, v1) - v_label (the loop's loss)
//   feasible[b]    every budget window holds (window w = x_w .. x_{w+h-1} has at most caps[w] ones)
//   objective[b]   the log-potential sum of the decision, the quantity the MAP maximises
//   counts[4]      ADDED to: variables compared, variables correct, feasible samples, samples equal to the label everywhere
//
// The reference reports only the first two.  The model is the one of pgm_datapath.hip: unary [N][2], pair [N-1][4] (row-major
// [x_i][x_{i+1}]), caps [N-h+1], each with a batch stride (0: shared by the batch).
//
// One wave per sample, PS_WAVES samples per workgroup per pass, the grid striding over the batch.  Lane l holds variable
// l + 64 j in chunk j.  Every load of a chunk (both logits, the label, both unary entries, the link's four entries) is independent of
// the decision, so they go out together; the decision then picks the terms.  The chunk's decisions are one ballot: its popcount
// is the number of ones, and the masks with their running counts go to LDS, where a window's sum is a difference of two prefix
// counts.  The objective is summed in f64 by every lane in the order of the MAP recursion (pgm_datapath.hip: u_0, then
// (acc + pair_{t-1}) + u_t), the terms broadcast one lane at a time, so scoring the MAP label gives fgnn_chain_budget_map's
// objective exactly.  The NLL is summed per lane in chunk order and then over the wave by an xor butterfly (fixed order; every
// lane ends with the same value).  Counts are per wave in registers, summed over the workgroup's waves in LDS and added to global
// memory with integer atomics (cdna_hip_programming.md Guideline 12): integer sums do not depend on arrival order.
#include "fgnn_common.h"
#include "fgnn_device.h"
#include <stdint.h>

#define PS_THREADS 256
#define PS_WAVES (PS_THREADS / 64)
#define PS_MAXN 1024
#define PS_MAXCH (PS_MAXN / 64)
#define PS_MAXGRID 1024

struct PsParams {
    const void* dec; int64_t d_sb, d_cs, d_vs;   // logits dec[b d_sb + c d_cs + i d_vs] or assignments dec[b d_sb + i d_vs]
    const int64_t* label; int64_t l_sb;          // [B][l_sb], variables contiguous
    const float* unary; int64_t u_sb;            // [B][N][2]
    const float* pair; int64_t p_sb;             // [B][N-1][4]
    const int32_t* caps; int64_t c_sb;           // [B][N-h+1]
    int32_t* correct; uint8_t* feasible; double* objective; double* nll;
    unsigned long long* counts;                  // [4]
    int64_t B;
    int N, h;
};

template <int DK>
__global__ __launch_bounds__(PS_THREADS) void chain_budget_score_kernel(const PsParams p) {
    __shared__ unsigned long long s_mask[PS_WAVES][PS_MAXCH + 1];   // chunk j's decisions, bit l = variable 64 j + l
    __shared__ int s_cum[PS_WAVES][PS_MAXCH + 1];                   // ones in the chunks before j
    __shared__ unsigned long long s_cnt[PS_WAVES][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = p.N, h = p.h, nch = (N + 63) >> 6, nwin = N - h + 1;
    unsigned long long c_cor = 0, c_feas = 0, c_exact = 0, c_live = 0;      // wave-uniform
    for (int64_t b0 = (int64_t)blockIdx.x * PS_WAVES; b0 < p.B; b0 += (int64_t)gridDim.x * PS_WAVES) {
        const int64_t b = b0 + wave;
        const bool live = b < p.B;         // a wave past the batch end runs along (barriers) and loads / writes nothing
        const int cap0 = live && lane < nwin ? p.caps[b * p.c_sb + lane] : 0x7fffffff;
        double obj = 0.0, nl = 0.0;
        int cor = 0, cum = 0;
        unsigned long long prev = 0;
        for (int j = 0; j < nch; ++j) {
            const int i = (j << 6) + lane;
            const bool on = live && i < N;
            float v0 = 0.f, v1 = 0.f, u0 = 0.f, u1 = 0.f, q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
            int64_t xv = 0, lab = 0;
            if (on) {
                const int64_t o = b * p.d_sb + i * p.d_vs;
                if (DK == FGNN_PGM_DEC_I64) xv = static_cast<const int64_t*>(p.dec)[o];
                else fgnn_pgm_logits<DK>(p.dec, o, p.d_cs, v0, v1);
                lab = fgnn_pgm_label(p.label, b, p.l_sb, i);
                const float* u = p.unary + b * p.u_sb + 2 * i;
                u0 = u[0]; u1 = u[1];
                if (i > 0) {
                    const float* q = p.pair + b * p.p_sb + 4 * (i - 1);
                    q0 = q[0]; q1 = q[1]; q2 = q[2]; q3 = q[3];
                }
            }
            int x;
            if (DK == FGNN_PGM_DEC_I64) {
                x = xv != 0;
            } else {
                x = fgnn_pgm_decide(v0, v1);
                const double a = v0, c = v1, mx = a > c ? a : c;
                const double lse = mx + log1p(exp(-fabs(a - c)));
                if (on) nl += lse - (lab != 0 ? c : a);
            }
            const bool eq = DK == FGNN_PGM_DEC_I64 ? xv == lab : (int64_t)x == lab;
            const unsigned long long m = __ballot(on && x);
            cor += __popcll(__ballot(on && eq));
            if (lane == 0) { s_mask[wave][j] = m; s_cum[wave][j] = cum; }
            cum += __popcll(m);
            // the objective's terms of variable i: unary[i][x_i] and, for i > 0, pair[i-1][2 x_{i-1} + x_i]
            const int xp = lane ? (int)((m >> (lane - 1)) & 1ull) : (int)(prev >> 63);
            const int k = 2 * xp + x;
            const float uu = x ? u1 : u0, pp = k == 0 ? q0 : k == 1 ? q1 : k == 2 ? q2 : q3;
            const int nj = N - (j << 6) < 64 ? N - (j << 6) : 64;
            for (int l = 0; l < nj; ++l) {
                if (j | l) obj += (double)fgnn_bcast(pp, l);
                obj += (double)fgnn_bcast(uu, l);
            }
            prev = m;
        }
        if (lane == 0) { s_mask[wave][nch] = 0; s_cum[wave][nch] = cum; }
        __syncthreads();
        bool bad = false;
        if (live) {
            for (int w = lane; w < nwin; w += 64) {        // ones in x_w .. x_{w+h-1} = prefix(w + h) - prefix(w)
                const int e = w + h;
                const int pw = s_cum[wave][w >> 6] + __popcll(s_mask[wave][w >> 6] & ((1ull << (w & 63)) - 1ull));
                const int pe = s_cum[wave][e >> 6] + __popcll(s_mask[wave][e >> 6] & ((1ull << (e & 63)) - 1ull));
                const int cap = w < 64 ? cap0 : p.caps[b * p.c_sb + w];
                bad |= pe - pw > cap;
            }
        }
        const bool feas = __ballot(bad) == 0ull;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) nl += __shfl_xor(nl, s);
        if (live) {
            if (lane == 0) {
                if (p.correct) p.correct[b] = cor;
                if (p.feasible) p.feasible[b] = feas ? 1 : 0;
                if (p.objective) p.objective[b] = obj;
                if (p.nll) p.nll[b] = nl;
            }
            c_live += 1;
            c_cor += (unsigned long long)cor;
            c_feas += feas;
            c_exact += cor == N;
        }
        __syncthreads();               // the next pass rewrites this wave's masks
    }
    if (!p.counts) return;             // (uniform: every thread leaves together)
    if (lane == 0) {
        s_cnt[wave][0] = c_live * (unsigned long long)N;
        s_cnt[wave][1] = c_cor;
        s_cnt[wave][2] = c_feas;
        s_cnt[wave][3] = c_exact;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < PS_WAVES; ++w) s += s_cnt[w][threadIdx.x];
        if (s) atomicAdd(p.counts + threadIdx.x, s);
    }
}

extern "C" int fgnn_chain_budget_score(const void* dec, int dec_kind, int64_t dec_sb, int64_t dec_cs, int64_t dec_vs,
                                       const int64_t* label, int64_t label_sb, const float* unary, int64_t unary_sb,
                                       const float* pair, int64_t pair_sb, const int32_t* caps, int64_t caps_sb, int64_t B, int N,
                                       int h, int32_t* correct, uint8_t* feasible, double* objective, double* nll, int64_t* counts,
                                       fgnn_stream_t stream) {
    if (dec_kind != FGNN_PGM_DEC_F32 && dec_kind != FGNN_PGM_DEC_BF16 && dec_kind != FGNN_PGM_DEC_I64)
        FGNN_FAIL(FGNN_EUNSUPPORTED, "chain_budget_score: decision kind %d", dec_kind);
    if (B < 0 || N < 0) FGNN_FAIL(FGNN_EINVAL, "chain_budget_score: negative size (B=%lld N=%d)", (long long)B, N);
    if (dec_sb < 0 || dec_cs < 0 || dec_vs < 0 || label_sb < 0 || unary_sb < 0 || pair_sb < 0 || caps_sb < 0)
        FGNN_FAIL(FGNN_EINVAL, "chain_budget_score: negative stride");
    if (N > PS_MAXN) FGNN_FAIL(FGNN_EUNSUPPORTED, "chain_budget_score: chain length N=%d above %d", N, PS_MAXN);
    if (h < 1 || h > N) FGNN_FAIL(FGNN_EUNSUPPORTED, "chain_budget_score: window h=%d outside 1..N=%d", h, N);
    if (dec_kind == FGNN_PGM_DEC_I64 && nll) FGNN_FAIL(FGNN_EINVAL, "chain_budget_score: nll needs logits, not assignments");
    if (B == 0) return FGNN_OK;
    if (!dec || !label || !unary || !pair || !caps) FGNN_FAIL(FGNN_EINVAL, "chain_budget_score: null pointer");
    const PsParams p = {dec, dec_sb, dec_cs, dec_vs, label, label_sb, unary, unary_sb, pair, pair_sb, caps, caps_sb,
                        correct, feasible, objective, nll, (unsigned long long*)counts, B, N, h};
    int64_t grid = (B + PS_WAVES - 1) / PS_WAVES;
    if (grid > PS_MAXGRID) grid = PS_MAXGRID;
    fgnn_note_kernel("chain_budget_score_kernel");
    void (*kernel)(PsParams);
    if (dec_kind == FGNN_PGM_DEC_F32) kernel = chain_budget_score_kernel<FGNN_PGM_DEC_F32>;
    else if (dec_kind == FGNN_PGM_DEC_BF16) kernel = chain_budget_score_kernel<FGNN_PGM_DEC_BF16>;
    else kernel = chain_budget_score_kernel<FGNN_PGM_DEC_I64>;
    return fgnn_launch("chain_budget_score", kernel, dim3((unsigned)grid), dim3(PS_THREADS), 0, fgnn_stream(stream), p);
}
