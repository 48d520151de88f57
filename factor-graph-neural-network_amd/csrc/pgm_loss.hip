// pgm_loss.hip — the labelling loss of the synthetic-PGM training scripts (/root/reference/train_syn_hop_factor.py:298-312,
// train_syn_pw_factor.py:298-312, train_syn_fixed_pw_hop.py:283-303):
//
//   loss[0]    F.cross_entropy(pred.view(-1, 2), label.view(-1)) = the mean over the B N variables of logsumexp(v0, v1) - v_label
//   counts[3]  ADDED to: variables, variables where argmax(pred) == label (the loop's all_correct), variables where
//              lp_label == label (its lp_correct): the per-step acc / lp_acc without a host read
//   glogits    gloss[0] / (B N) (softmax_c - [c == label])
//
// The logits are read through their strides as pgm_eval.hip reads them (a model's [B, 2, N, 1] output as it is; the scripts'
// squeeze / permute / contiguous copy is not made), by the same helpers (fgnn_device.h: fgnn_pgm_logits, fgnn_pgm_label,
// fgnn_pgm_decide).  One thread per variable.  Every summand is formed in f64 from the stored values as a softplus of the logit
// difference, logsumexp(v0, v1) - v_label = softplus(v_other - v_label) = max(t, 0) + log1p(exp(-|t|)): nothing is lost when the
// logits are far apart.  A thread sums its variables in grid-stride order, a wave by an xor butterfly, a workgroup its four waves in
// order, and a second one-thread launch the workgroups' partials in order and rounds once to f32: the grid is a function of B N
// alone, so the loss is bit-reproducible.  Counts are integer atomics (cdna_hip_programming.md Guideline 12).
#include "fgnn_common.h"
#include "fgnn_device.h"
#include <math.h>
#include <stdint.h>
#include <type_traits>

#define PL_THREADS 256
#define PL_WAVES (PL_THREADS / 64)
#define PL_MAXN 1024
#define PL_MAXGRID 256

struct PlParams {
    const void* logits; int64_t sb, cs, vs;
    const int64_t* label; int64_t l_sb;
    const int64_t* lp; int64_t lp_sb;            // or NULL
    double* part;                                // [gridDim.x]
    unsigned long long* counts;                  // [3] or NULL
    int64_t total;                               // B N
    int N;
};

template <int DK>
__global__ __launch_bounds__(PL_THREADS) void pgm_loss_fwd_kernel(const PlParams p) {
    __shared__ double s_sum[PL_WAVES];
    __shared__ unsigned long long s_cnt[PL_WAVES][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    unsigned long long c_var = 0, c_cor = 0, c_lp = 0;       // wave-uniform
    // (every lane of a wave runs the same number of passes: the ballots below see the whole wave)
    for (int64_t e0 = (int64_t)blockIdx.x * PL_THREADS + (wave << 6); e0 < p.total; e0 += (int64_t)gridDim.x * PL_THREADS) {
        const int64_t e = e0 + lane;
        const bool on = e < p.total;
        bool eq = false, lpeq = false;
        if (on) {
            const int64_t b = e / p.N;
            const int i = (int)(e - b * p.N);
            float v0, v1;
            fgnn_pgm_logits<DK>(p.logits, b * p.sb + i * p.vs, p.cs, v0, v1);
            const int64_t lab = fgnn_pgm_label(p.label, b, p.l_sb, i);
            const double t = lab != 0 ? (double)v0 - (double)v1 : (double)v1 - (double)v0;      // v_other - v_label
            acc += (t > 0.0 ? t : 0.0) + log1p(exp(-fabs(t)));
            eq = (int64_t)fgnn_pgm_decide(v0, v1) == lab;
            if (p.lp) lpeq = fgnn_pgm_label(p.lp, b, p.lp_sb, i) == lab;
        }
        c_var += __popcll(__ballot(on));
        c_cor += __popcll(__ballot(eq));
        c_lp += __popcll(__ballot(lpeq));
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
    if (lane == 0) {
        s_sum[wave] = acc;
        s_cnt[wave][0] = c_var; s_cnt[wave][1] = c_cor; s_cnt[wave][2] = c_lp;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < PL_WAVES; ++w) s += s_sum[w];
        p.part[blockIdx.x] = s;
    }
    if (p.counts && threadIdx.x < 3 && (threadIdx.x < 2 || p.lp)) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < PL_WAVES; ++w) s += s_cnt[w][threadIdx.x];
        if (s) atomicAdd(p.counts + threadIdx.x, s);
    }
}

// the partials in workgroup order, the mean, one rounding
__global__ void pgm_loss_final_kernel(const double* __restrict__ part, int npart, int64_t total, float* __restrict__ loss) {
    double s = 0.0;
    for (int i = 0; i < npart; ++i) s += part[i];
    loss[0] = (float)(s / (double)total);
}

struct PlBwdParams {
    const void* logits; int64_t sb, cs, vs;
    const int64_t* label; int64_t l_sb;
    const float* gloss;
    void* glogits; int64_t g_sb, g_cs, g_vs;
    int64_t total;
    int N;
};

template <int DK>
__global__ __launch_bounds__(PL_THREADS) void pgm_loss_bwd_kernel(const PlBwdParams p) {
    typedef typename std::conditional<DK == FGNN_PGM_DEC_F32, float, bf16_t>::type T;
    const double g = (double)p.gloss[0] / (double)p.total;
    for (int64_t e = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; e < p.total; e += (int64_t)gridDim.x * PL_THREADS) {
        const int64_t b = e / p.N;
        const int i = (int)(e - b * p.N);
        float v0, v1;
        fgnn_pgm_logits<DK>(p.logits, b * p.sb + i * p.vs, p.cs, v0, v1);
        const bool one = fgnn_pgm_label(p.label, b, p.l_sb, i) != 0;
        // softmax_other = sigmoid(t), t = v_other - v_label; softmax_label - 1 = -softmax_other: no cancellation at either end
        const double t = one ? (double)v0 - (double)v1 : (double)v1 - (double)v0;
        const double ex = exp(-fabs(t));
        const double so = g * (t >= 0.0 ? 1.0 / (1.0 + ex) : ex / (1.0 + ex));
        T* out = static_cast<T*>(p.glogits) + b * p.g_sb + i * p.g_vs;
        fgnn_st(out, (float)(one ? so : -so));
        fgnn_st(out + p.g_cs, (float)(one ? -so : so));
    }
}

static int pl_check(const char* what, const void* logits, int kind, int64_t sb, int64_t cs, int64_t vs, const int64_t* label,
                    int64_t label_sb, int64_t B, int N) {
    if (kind != FGNN_PGM_DEC_F32 && kind != FGNN_PGM_DEC_BF16) FGNN_FAIL(FGNN_EUNSUPPORTED, "%s: logit kind %d", what, kind);
    if (B < 0 || N < 0) FGNN_FAIL(FGNN_EINVAL, "%s: negative size (B=%lld N=%d)", what, (long long)B, N);
    if (sb < 0 || cs < 0 || vs < 0 || label_sb < 0) FGNN_FAIL(FGNN_EINVAL, "%s: negative stride", what);
    if (N < 1 || N > PL_MAXN) FGNN_FAIL(FGNN_EUNSUPPORTED, "%s: chain length N=%d outside 1..%d", what, N, PL_MAXN);
    if (!logits || !label) FGNN_FAIL(FGNN_EINVAL, "%s: null pointer", what);
    return FGNN_OK;
}

static unsigned pl_grid(int64_t total) {
    int64_t g = (total + PL_THREADS - 1) / PL_THREADS;
    return (unsigned)(g > PL_MAXGRID ? PL_MAXGRID : g < 1 ? 1 : g);
}

extern "C" int64_t fgnn_pgm_loss_workspace_bytes(void) { return (int64_t)PL_MAXGRID * sizeof(double); }

extern "C" int fgnn_pgm_loss_forward(const void* logits, int kind, int64_t sb, int64_t cs, int64_t vs, const int64_t* label,
                                     int64_t label_sb, const int64_t* lp_label, int64_t lp_sb, int64_t B, int N, float* loss,
                                     int64_t* counts, void* workspace, int64_t workspace_bytes, fgnn_stream_t stream) {
    if (int rc = pl_check("pgm_loss_forward", logits, kind, sb, cs, vs, label, label_sb, B, N)) return rc;
    if (lp_sb < 0) FGNN_FAIL(FGNN_EINVAL, "pgm_loss_forward: negative stride");
    if (!loss) FGNN_FAIL(FGNN_EINVAL, "pgm_loss_forward: null pointer");
    if (!workspace || workspace_bytes < fgnn_pgm_loss_workspace_bytes() || ((uintptr_t)workspace & 7))
        FGNN_FAIL(FGNN_EINVAL, "pgm_loss_forward: an 8-byte aligned workspace of fgnn_pgm_loss_workspace_bytes() bytes needed");
    hipStream_t st = fgnn_stream(stream);
    const int64_t total = B * N;
    const unsigned grid = pl_grid(total);
    double* part = (double*)workspace;
    if (B > 0) {
        const PlParams p = {logits, sb, cs, vs, label, label_sb, lp_label, lp_sb, part, (unsigned long long*)counts, total, N};
        fgnn_note_kernel("pgm_loss_fwd_kernel");
        const auto kernel = kind == FGNN_PGM_DEC_F32 ? pgm_loss_fwd_kernel<FGNN_PGM_DEC_F32> : pgm_loss_fwd_kernel<FGNN_PGM_DEC_BF16>;
        if (int rc = fgnn_launch("pgm_loss forward", kernel, dim3(grid), dim3(PL_THREADS), 0, st, p)) return rc;
    }
    // B = 0: no partials, and the mean of nothing is written as 0
    return fgnn_launch("pgm_loss forward", pgm_loss_final_kernel, dim3(1), dim3(1), 0, st, part, B > 0 ? (int)grid : 0, B > 0 ? total : 1, loss);
}

extern "C" int fgnn_pgm_loss_backward(const void* logits, int kind, int64_t sb, int64_t cs, int64_t vs, const int64_t* label,
                                      int64_t label_sb, const float* gloss, int64_t B, int N, void* glogits, int64_t g_sb,
                                      int64_t g_cs, int64_t g_vs, fgnn_stream_t stream) {
    if (int rc = pl_check("pgm_loss_backward", logits, kind, sb, cs, vs, label, label_sb, B, N)) return rc;
    if (g_sb < 0 || g_cs < 0 || g_vs < 0) FGNN_FAIL(FGNN_EINVAL, "pgm_loss_backward: negative stride");
    if (!gloss || !glogits) FGNN_FAIL(FGNN_EINVAL, "pgm_loss_backward: null pointer");
    if (B == 0) return FGNN_OK;
    const int64_t total = B * N;
    const PlBwdParams p = {logits, sb, cs, vs, label, label_sb, gloss, glogits, g_sb, g_cs, g_vs, total, N};
    fgnn_note_kernel("pgm_loss_bwd_kernel");
    int64_t g = (total + PL_THREADS - 1) / PL_THREADS;
    if (g > 4096) g = 4096;
    const auto kernel = kind == FGNN_PGM_DEC_F32 ? pgm_loss_bwd_kernel<FGNN_PGM_DEC_F32> : pgm_loss_bwd_kernel<FGNN_PGM_DEC_BF16>;
    return fgnn_launch("pgm_loss backward", kernel, dim3((unsigned)g), dim3(PL_THREADS), 0, fgnn_stream(stream), p);
}
