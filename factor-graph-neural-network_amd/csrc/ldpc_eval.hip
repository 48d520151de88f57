// ldpc_eval.hip — the decoding-quality accounting of the reference's LDPC test loop, in one launch per batch:
//
//   acc_cnt[csnr][b] / acc_tot[csnr][b]   bits right / compared per class (SNR of bit 0 within 1e-3 of a grid value, sigma_b.long()
//                                         equal to a grid value), /root/reference/train_ldpc.py:289-327
//   acc_seq / tot                         the same over every word (the overall bit error rate)
//
// plus word (frame) errors beside them.  Decisions are a model's logits (bit = v >= 0, train_ldpc.py:302) or a decoder's hard
// decisions (bit = v != 0); labels the reference's int64 `gts` or the encoder's bytes.  The counts are ADDED to `counts`, so a whole
// test set accumulates on the device and the host reads it once.
//
// One wave per word (LE_UNROLL words per pass, their loads issued together): lane j compares bit j (+ 64 per chunk), the word's
// error count is the popcount of the wave's ballot.  Counters are per wave in LDS (one lane writes them: no LDS atomics), summed
// over the workgroup's waves at the end and added to global memory once per non-zero counter per workgroup with integer atomics
// (cdna_hip_programming.md Guideline 12): integer sums do not depend on arrival order, so the counts are deterministic.  The grid
// is capped at LE_MAXGRID workgroups (at most that many adds per counter) and strides over the batch.
#include "fgnn_common.h"
#include <stdint.h>

#define LE_THREADS 256
#define LE_WAVES (LE_THREADS / 64)
#define LE_UNROLL 4
#define LE_MAXGRID 256
#define LE_MAXCLASSES 256
#define LE_MAXBITS 1024

struct LeParams {
    const void* dec;             // [B][dec_sb] f32 / bf16 logits or bytes
    const void* label;           // [B][label_sb] int64 or bytes
    const float* snr_db;         // snr_db[b * snr_sb]
    const float* sigma_b;        // [B]
    const float* snr_grid;       // [n_snr]
    const int32_t* sigma_grid;   // [n_sigma]
    unsigned long long* counts;  // [n_snr * n_sigma + 1][4]
    int64_t dec_sb, label_sb, snr_sb, B;
    int nbits, n_snr, n_sigma;
};

template <int DK>
__device__ __forceinline__ int le_bit(const void* dec, int64_t i) {
    if (DK == FGNN_DEC_F32) return static_cast<const float*>(dec)[i] >= 0.f;
    if (DK == FGNN_DEC_BF16) return fgnn_ld(static_cast<const bf16_t*>(dec) + i) >= 0.f;
    return static_cast<const uint8_t*>(dec)[i] != 0;
}

template <int LK>
__device__ __forceinline__ int64_t le_label(const void* label, int64_t i) {
    if (LK == FGNN_LABEL_I64) return static_cast<const int64_t*>(label)[i];
    return static_cast<const uint8_t*>(label)[i];
}

// class row of a word: SNR-major (snr index * n_sigma + sigma index), -1 when it matches no class
__device__ __forceinline__ int le_class(float snr, float sb, const float* sg, const int* bg, int n_snr, int n_sigma) {
    int si = -1, bi = -1;
    for (int k = 0; k < n_snr; ++k)
        if (fabsf(snr - sg[k]) < 1e-3f) { si = k; break; }
    if (sb > -9.0e18f && sb < 9.0e18f) {            // sigma_b.long(): truncation; NaN / out of range matches nothing
        const int64_t t = (int64_t)sb;
        for (int k = 0; k < n_sigma; ++k)
            if ((int64_t)bg[k] == t) { bi = k; break; }
    }
    return si < 0 || bi < 0 ? -1 : si * n_sigma + bi;
}

template <int DK, int LK>
__global__ __launch_bounds__(LE_THREADS) void ldpc_error_counts_kernel(const LeParams p) {
    extern __shared__ unsigned long long le_cnt[];  // [LE_WAVES][nrow][4]
    __shared__ float sg[LE_MAXCLASSES];
    __shared__ int bg[LE_MAXCLASSES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nrow = p.n_snr * p.n_sigma + 1, nb = p.nbits;
    for (int i = tid; i < LE_WAVES * nrow * 4; i += LE_THREADS) le_cnt[i] = 0;
    for (int i = tid; i < p.n_snr; i += LE_THREADS) sg[i] = p.snr_grid[i];
    for (int i = tid; i < p.n_sigma; i += LE_THREADS) bg[i] = p.sigma_grid[i];
    __syncthreads();
    unsigned long long* my = le_cnt + wave * nrow * 4;
    const int64_t B = p.B, step = (int64_t)gridDim.x * LE_WAVES * LE_UNROLL;
    for (int64_t b0 = ((int64_t)blockIdx.x * LE_WAVES + wave) * LE_UNROLL; b0 < B; b0 += step) {
        int errs[LE_UNROLL], row[LE_UNROLL];
#pragma unroll
        for (int u = 0; u < LE_UNROLL; ++u) {      // the class first: its loads go out with the decisions', not after the ballots
            const int64_t b = b0 + u;
            errs[u] = 0;
            row[u] = b < B ? le_class(p.snr_db[b * p.snr_sb], p.sigma_b[b], sg, bg, p.n_snr, p.n_sigma) : -1;
        }
        for (int c0 = 0; c0 < nb; c0 += 64) {
            const int j = c0 + lane;
            int e[LE_UNROLL];
#pragma unroll
            for (int u = 0; u < LE_UNROLL; ++u) {
                const int64_t b = b0 + u;
                e[u] = b < B && j < nb && (int64_t)le_bit<DK>(p.dec, b * p.dec_sb + j) != le_label<LK>(p.label, b * p.label_sb + j);
            }
#pragma unroll
            for (int u = 0; u < LE_UNROLL; ++u) errs[u] += __popcll(__ballot(e[u]));
        }
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < LE_UNROLL; ++u) {
                const int64_t b = b0 + u;
                if (b >= B) break;
                const int rows[2] = {row[u], nrow - 1};
                for (int r = 0; r < 2; ++r) {
                    if (rows[r] < 0) continue;
                    unsigned long long* c = my + rows[r] * 4;
                    c[0] += (unsigned long long)nb;
                    c[1] += (unsigned long long)errs[u];
                    c[2] += 1ull;
                    c[3] += errs[u] != 0;
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < nrow * 4; i += LE_THREADS) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < LE_WAVES; ++w) s += le_cnt[w * nrow * 4 + i];
        if (s) atomicAdd(p.counts + i, s);
    }
}

extern "C" int fgnn_ldpc_error_counts(const void* dec, int dec_kind, int64_t dec_sb, const void* label, int label_kind, int64_t label_sb,
                                      const float* snr_db, int64_t snr_sb, const float* sigma_b, int64_t B, int nbits,
                                      const float* snr_grid, int n_snr, const int32_t* sigma_grid, int n_sigma, int64_t* counts,
                                      fgnn_stream_t stream) {
    if (dec_kind != FGNN_DEC_F32 && dec_kind != FGNN_DEC_BF16 && dec_kind != FGNN_DEC_U8)
        FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_error_counts: decision kind %d", dec_kind);
    if (label_kind != FGNN_LABEL_I64 && label_kind != FGNN_LABEL_U8)
        FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_error_counts: label kind %d", label_kind);
    if (nbits < 1 || nbits > LE_MAXBITS) FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_error_counts: nbits=%d (1..%d)", nbits, LE_MAXBITS);
    if (n_snr < 1 || n_sigma < 1 || (int64_t)n_snr * n_sigma > LE_MAXCLASSES)
        FGNN_FAIL(FGNN_EUNSUPPORTED, "ldpc_error_counts: %d x %d classes (1..%d)", n_snr, n_sigma, LE_MAXCLASSES);
    if (B < 0 || dec_sb < 0 || label_sb < 0 || snr_sb < 0)
        FGNN_FAIL(FGNN_EINVAL, "ldpc_error_counts: negative size or stride");
    if (B == 0) return FGNN_OK;
    if (!dec || !label || !snr_db || !sigma_b || !snr_grid || !sigma_grid || !counts)
        FGNN_FAIL(FGNN_EINVAL, "ldpc_error_counts: null pointer");
    const LeParams p = {dec, label, snr_db, sigma_b, snr_grid, sigma_grid, (unsigned long long*)counts, dec_sb, label_sb, snr_sb, B,
                        nbits, n_snr, n_sigma};
    int64_t grid = (B + LE_WAVES * LE_UNROLL - 1) / (LE_WAVES * LE_UNROLL);
    if (grid > LE_MAXGRID) grid = LE_MAXGRID;
    const size_t lds = (size_t)LE_WAVES * (n_snr * n_sigma + 1) * 4 * sizeof(unsigned long long);
    fgnn_note_kernel("ldpc_error_counts_kernel");
    void (*kernel)(LeParams);
    if (label_kind == FGNN_LABEL_I64) {
        if (dec_kind == FGNN_DEC_F32) kernel = ldpc_error_counts_kernel<FGNN_DEC_F32, FGNN_LABEL_I64>;
        else if (dec_kind == FGNN_DEC_BF16) kernel = ldpc_error_counts_kernel<FGNN_DEC_BF16, FGNN_LABEL_I64>;
        else kernel = ldpc_error_counts_kernel<FGNN_DEC_U8, FGNN_LABEL_I64>;
    } else {
        if (dec_kind == FGNN_DEC_F32) kernel = ldpc_error_counts_kernel<FGNN_DEC_F32, FGNN_LABEL_U8>;
        else if (dec_kind == FGNN_DEC_BF16) kernel = ldpc_error_counts_kernel<FGNN_DEC_BF16, FGNN_LABEL_U8>;
        else kernel = ldpc_error_counts_kernel<FGNN_DEC_U8, FGNN_LABEL_U8>;
    }
    return fgnn_launch("ldpc_error_counts", kernel, dim3((unsigned)grid), dim3(LE_THREADS), lds, fgnn_stream(stream), p);
}
