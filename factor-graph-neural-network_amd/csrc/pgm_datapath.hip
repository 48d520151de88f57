// pgm_datapath.hip — the synthetic-PGM data path on the GPU: exact MAP labels and the reference's random models.
//
//   fgnn_chain_budget_map   exact MAP of a binary chain with sliding-window budget factors — what
//                           `PFactorGraph.solve(branch_and_bound=True)` (AD3) returns for the models of
//                           /root/reference/lib/data/random_pgm.py:20-48, random_pgm_pw.py:28-45,75-85, random_pgm_hop.py:28-45,111-125
//                           and their NoHop variants
//   fgnn_pgm_sample_rng     those random models themselves (random_pgm*.py: `__getitem__`), drawn in the kernel, with their
//                           model inputs and the same solver's labels
//
// The model.  N binary variables x_0 .. x_{N-1}; unary log-potentials unary[i][x_i]; a 2x2 log-potential pair[i][x_i][x_{i+1}]
// on each link (row-major: pair[i][2 x_i + x_{i+1}], how the reference flattens `pws_to_right.reshape(-1)`; AD3's own order for
// dense factors is not checked here, and it matters only for an asymmetric table such as the `raw` family's [0, .1, .2, 1]);
// and on every window w = 0 .. N-h of h consecutive variables x_w .. x_{w+h-1} a budget: at most cap[w] ones (cap >= h: no
// constraint).  Maximise the sum of the log-potentials.
//
// The DP.  State after position t = the last h-1 bits, s = sum_k x_{t-k} 2^k (bit 0 the newest; bits of positions < 0 are 0).
// Adding b = x_{t+1}: s' = ((s << 1) | b) & (S-1), S = 2^(h-1); s' has the two predecessors p_d = (d << (h-2)) | (s' >> 1), d the
// dropped oldest bit.  The window ending at t+1 is exactly (bits of p_d, b), so the move is allowed iff popcount(p_d) + b <=
// cap[t+1-h+1] once t+1 >= h-1; before that the dropped bit is a position < 0 and must be 0 (d = 0 only).  Start: V(0) = unary[0][0],
// V(1) = unary[0][1], every other state infeasible.  Exact (Viterbi on 2^(h-1) states), no branch and bound.
//
// Arithmetic and ties (fixed, restated in tests/pgm_map_oracle.py): scores are f64; a candidate is (V[p_d] + pair) + unary, in that
// order; d = 1 is taken only when its score is strictly greater (d = 0 on ties); at the end the lowest state index among the maxima.
// An infeasible move scores -inf.  Every cap >= 0 keeps all-zeros feasible; with a negative cap the objective may be -inf and the
// labels are then the traceback of the lowest state.
//
// Layout: one wave64 per sample, `spw` samples per workgroup (sized from the LDS footprint).  Lane l holds the states l + 64 j
// (S < 64: lanes >= S idle).  The scores live in a double-buffered LDS array, the backpointers are one bit per (t, s'), gathered
// with __ballot (N S / 8 bytes: 960 B at N = 30, h = 9), and one lane traces back.
#include "fgnn_common.h"
#include "fgnn_philox.h"
#include <stdint.h>

#define CB_MAX_H 13
#define CB_LDS_MAX (160 * 1024)
#define CB_LDS_TARGET (64 * 1024)       // workgroup footprint the samples-per-workgroup choice aims under
#define CB_MAX_SPW 4

extern __shared__ __attribute__((aligned(16))) unsigned char cb_lds[];

enum { CB_RAW = 0, CB_PWS = 1, CB_HOPS = 2 };

struct CbParams {
    const float* unary; int64_t u_sb;      // [B][N][2]      (u_sb = 0: shared by the batch)
    const float* pair; int64_t p_sb;       // [B][N-1][4]
    const int32_t* caps; int64_t c_sb;     // [B][N-h+1]
    int family, cap;                       // sampler: CB_*, fixed budget of the raw / pws families
    float trans[4];                        // sampler, raw family: the fixed link table
    unsigned long long seed, offset;       // sampler: Philox key and counter offset
    float *node, *pws, *hops;              // sampler outputs [B][2][N], [B][4][N], [B][h][N] (NULL: not written)
    int64_t* labels;                       // [B][N]
    double* objective;                     // [B] or NULL
    int64_t B;
    int N, h, spw, sample_bytes;
};

// per-sample LDS footprint: V (2 S doubles), backpointers (N rows of W words), unary 2N, pair 4(N-1), caps N; -1 outside the family
static int64_t cb_sample_bytes(int N, int h) {
    if (h < 2 || h > CB_MAX_H || N < h) return -1;
    const int64_t S = 1ll << (h - 1), W = S >= 64 ? S / 64 : 1;
    const int64_t bytes = 16 * S + 8 * (int64_t)N * W + 4 * (2 * (int64_t)N + 4 * ((int64_t)N - 1) + N);
    const int64_t r = (bytes + 15) / 16 * 16;
    return r <= CB_LDS_MAX ? r : -1;
}

template <bool SAMPLER>
__global__ __launch_bounds__(64 * CB_MAX_SPW) void chain_budget_map_kernel(const CbParams p) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int N = p.N, h = p.h, S = 1 << (h - 1), half = S >> 1, W = S >= 64 ? S >> 6 : 1;
    const int64_t b = (int64_t)blockIdx.x * p.spw + wave;
    const bool live = b < p.B;
    const int64_t bb = live ? b : p.B - 1;         // a wave past the batch end runs along (barriers) and writes nothing
    unsigned char* base = cb_lds + (int64_t)wave * p.sample_bytes;
    double* V0 = (double*)base;
    double* V1 = V0 + S;
    unsigned long long* bp = (unsigned long long*)(V1 + S);      // [N][W]
    float* un = (float*)(bp + (int64_t)N * W);                  // [N][2]
    float* pr = un + 2 * N;                                     // [N-1][4]
    int* cp = (int*)(pr + 4 * (N - 1));                         // window w's cap = cp[w + coff]
    int coff = 0;

    // ---- stage the sample's potentials in LDS ----
    if (!SAMPLER) {
        const float* u = p.unary + bb * p.u_sb;
        const float* q = p.pair + bb * p.p_sb;
        const int32_t* c = p.caps + bb * p.c_sb;
        for (int k = lane; k < 2 * N; k += 64) un[k] = u[k];
        for (int k = lane; k < 4 * (N - 1); k += 64) pr[k] = q[k];
        for (int k = lane; k < N - h + 1; k += 64) cp[k] = c[k];
    } else {
        // Word w of sample b = philox(counter (b, w >> 2, offset lo, offset hi), key (seed lo, seed hi))[w & 3], in the reference's
        // draw order: lops[i][c] at w = 2i + c (U[0,1) = (r >> 8) 2^-24), then the link bonus pair[i][1][1] = 2 U for i < N-1 (pws,
        // hops), then the per-position caps 1 + floor(r (h-1) / 2^32) for i < N (hops).  Restated in tests/pgm_map_oracle.py.
        const int fam = p.family;
        const int nw = 2 * N + (fam != CB_RAW ? N - 1 : 0) + (fam == CB_HOPS ? N : 0);
        for (int k = lane; k < 4 * (N - 1); k += 64) {
            const int s = k & 3;
            if (fam == CB_RAW) pr[k] = p.trans[s];
            else if (s != 3) pr[k] = 0.f;
        }
        if (fam != CB_HOPS)
            for (int k = lane; k < N - h + 1; k += 64) cp[k] = p.cap;
        else
            coff = h >> 1;
        for (int qd = lane; qd < (nw + 3) >> 2; qd += 64) {
            unsigned r[4];
            ld_philox((unsigned)bb, (unsigned)qd, (unsigned)p.offset, (unsigned)(p.offset >> 32), (unsigned)p.seed,
                      (unsigned)(p.seed >> 32), r);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int w = 4 * qd + k;
                if (w >= nw) break;
                const float uf = (float)(r[k] >> 8) * 5.9604644775390625e-08f;
                if (w < 2 * N) un[w] = uf;
                else if (w < 3 * N - 1) pr[4 * (w - 2 * N) + 3] = 2.f * uf;
                else cp[w - (3 * N - 1)] = 1 + (int)(((unsigned long long)r[k] * (unsigned)(h - 1)) >> 32);
            }
        }
    }
    __syncthreads();

    if (SAMPLER && live) {      // the model inputs in the layouts train_syn_*.py feed to factor_mpnn
        float* node = p.node + b * 2 * N;                                            // [2][N] = lops^T
        for (int o = lane; o < 2 * N; o += 64) { const int c = o / N, i = o - c * N; node[o] = un[2 * i + c]; }
        if (p.pws) {                                                                 // [4][N]: the to-right link, zero at N-1
            float* pw = p.pws + b * 4 * N;
            for (int o = lane; o < 4 * N; o += 64) { const int k = o / N, i = o - k * N; pw[o] = i < N - 1 ? pr[4 * i + k] : 0.f; }
        }
        if (p.hops) {                                                                // [h][N]: one-hot cap, h-1 at the borders
            float* hp = p.hops + b * (int64_t)h * N;
            const int hh = h >> 1;
            for (int o = lane; o < h * N; o += 64) {
                const int k = o / N, i = o - k * N;
                const int hot = (i >= hh && i < N - hh) ? cp[i] : h - 1;
                hp[o] = k == hot ? 1.f : 0.f;
            }
        }
    }

    // ---- forward: V_t over the S states ----
    const double NEG = -__builtin_inf();
    for (int j = 0; j < W; ++j) {
        const int s = lane + 64 * j;
        if (s < S) V0[s] = s < 2 ? (double)un[s] : NEG;
    }
    __syncthreads();
    double *Vp = V0, *Vc = V1;
    for (int t = 1; t < N; ++t) {
        const bool chk = t >= h - 1;
        const int cap = chk ? cp[t - h + 1 + coff] : 0;
        const double u0 = (double)un[2 * t], u1 = (double)un[2 * t + 1];
        const float* pt = pr + 4 * (t - 1);
        for (int j = 0; j < W; ++j) {
            const int s = lane + 64 * j;
            bool take = false;
            if (s < S) {
                const int bit = s & 1, hi = s >> 1, pa = hi, pb = hi | half, pc = __popc(hi);
                const double ub = bit ? u1 : u0;
                double c0 = (Vp[pa] + (double)pt[((pa & 1) << 1) | bit]) + ub;
                double c1 = (Vp[pb] + (double)pt[((pb & 1) << 1) | bit]) + ub;
                if (chk && pc + bit > cap) c0 = NEG;
                if (!chk || pc + 1 + bit > cap) c1 = NEG;
                take = c1 > c0;
                Vc[s] = take ? c1 : c0;
            }
            const unsigned long long m = __ballot(take);
            if (lane == 0) bp[t * W + j] = m;
        }
        __syncthreads();
        double* tmp = Vp; Vp = Vc; Vc = tmp;
    }

    // ---- argmax (lowest state among the maxima), then one lane traces back ----
    double best = NEG;
    int arg = 0x7fffffff;
    for (int j = 0; j < W; ++j) {
        const int s = lane + 64 * j;
        if (s < S) {
            const double v = Vp[s];
            if (v > best || arg == 0x7fffffff) { best = v; arg = s; }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(best, m);
        const int oa = __shfl_xor(arg, m);
        if (ov > best || (ov == best && oa < arg)) { best = ov; arg = oa; }
    }
    if (live && lane == 0) {
        int64_t* lab = p.labels + b * N;
        int s = arg;
        for (int t = N - 1; t >= 1; --t) {
            lab[t] = s & 1;
            const int d = (int)((bp[t * W + (s >> 6)] >> (s & 63)) & 1ull);
            s = (d ? half : 0) | (s >> 1);
        }
        lab[0] = s & 1;
        if (p.objective) p.objective[b] = best;
    }
}

extern "C" int64_t fgnn_chain_budget_map_lds_bytes(int N, int h) {
    const int64_t r = cb_sample_bytes(N, h);
    if (r < 0) {
        if (h < 2 || h > CB_MAX_H) fgnn_set_error("chain_budget_map: window h=%d outside 2..%d", h, CB_MAX_H);
        else if (N < h) fgnn_set_error("chain_budget_map: chain length N=%d shorter than the window h=%d", N, h);
        else fgnn_set_error("chain_budget_map: N=%d h=%d needs more than %d bytes of LDS per sample", N, h, CB_LDS_MAX);
    }
    return r;
}

static int cb_launch(bool sampler, CbParams& p, hipStream_t st) {
    const int64_t per = fgnn_chain_budget_map_lds_bytes(p.N, p.h);
    if (per < 0) return FGNN_EUNSUPPORTED;
    if (p.B < 0 || p.B > 0x7fffffffll) FGNN_FAIL(FGNN_EINVAL, "chain_budget_map: batch %lld outside 0 .. 2^31-1", (long long)p.B);
    if (p.B == 0) return FGNN_OK;
    if (!p.labels) FGNN_FAIL(FGNN_EINVAL, "chain_budget_map: null labels");
    int spw = (int)(CB_LDS_TARGET / per);
    if (spw > CB_MAX_SPW) spw = CB_MAX_SPW;
    if (spw < 1) spw = 1;
    if (spw > p.B) spw = (int)p.B;
    p.spw = spw;
    p.sample_bytes = (int)per;
    const int lds = spw * (int)per;
    const auto kernel = sampler ? chain_budget_map_kernel<true> : chain_budget_map_kernel<false>;
    fgnn_note_kernel(sampler ? "chain_budget_map_kernel<sampler>" : "chain_budget_map_kernel");
    const unsigned grid = (unsigned)((p.B + spw - 1) / spw);
    return fgnn_launch("chain_budget_map", kernel, dim3(grid), dim3(64 * spw), lds, st, p);
}

extern "C" int fgnn_chain_budget_map(const float* unary, int64_t unary_sb, const float* pair, int64_t pair_sb, const int32_t* caps,
                                     int64_t caps_sb, int64_t B, int N, int h, int64_t* labels, double* objective,
                                     fgnn_stream_t stream) {
    if (B > 0 && (!unary || !pair || !caps)) FGNN_FAIL(FGNN_EINVAL, "chain_budget_map: null pointer");
    if (unary_sb < 0 || pair_sb < 0 || caps_sb < 0) FGNN_FAIL(FGNN_EINVAL, "chain_budget_map: negative batch stride");
    CbParams p = {};
    p.unary = unary; p.u_sb = unary_sb;
    p.pair = pair; p.p_sb = pair_sb;
    p.caps = caps; p.c_sb = caps_sb;
    p.labels = labels; p.objective = objective;
    p.B = B; p.N = N; p.h = h;
    return cb_launch(false, p, fgnn_stream(stream));
}

extern "C" int fgnn_pgm_sample_rng(int family, uint64_t seed, uint64_t offset, int64_t B, int N, int h, int cap,
                                   const float* transition, float* node, float* pws, float* hops, int64_t* labels,
                                   double* objective, fgnn_stream_t stream) {
    if (family < CB_RAW || family > CB_HOPS) FGNN_FAIL(FGNN_EINVAL, "pgm_sample: unknown family %d", family);
    if (B > 0 && !node) FGNN_FAIL(FGNN_EINVAL, "pgm_sample: null node feature");
    if (family == CB_RAW && !transition) FGNN_FAIL(FGNN_EINVAL, "pgm_sample: the raw family needs a transition table");
    if (family == CB_HOPS && B > 0 && (!pws || !hops)) FGNN_FAIL(FGNN_EINVAL, "pgm_sample: the hops family writes pws and hops");
    if (family == CB_PWS && B > 0 && !pws) FGNN_FAIL(FGNN_EINVAL, "pgm_sample: the pws family writes pws");
    CbParams p = {};
    p.family = family; p.cap = cap;
    if (transition) for (int k = 0; k < 4; ++k) p.trans[k] = transition[k];
    p.seed = seed; p.offset = offset;
    p.node = node;
    p.pws = family != CB_RAW ? pws : nullptr;
    p.hops = family == CB_HOPS ? hops : nullptr;
    p.labels = labels; p.objective = objective;
    p.B = B; p.N = N; p.h = h;
    return cb_launch(true, p, fgnn_stream(stream));
}
