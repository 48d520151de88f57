// ldpc_nms.h — what the two schedules of the learned min-sum decoder share (ldpc_nms.hip: flooding; ldpc_nms_layered.hip: layered):
// the limits, the launch parameters, the weight index, the record and the argument checks of the entry points.  Both sources are
// built with -ffp-contract=off.
//
// Record (train mode), per word b and iteration t three planes of M 32-bit values, plane k of check m at
// ((b * n_iter + t - 1) * 3 + k) * M + m:
//   plane 0  m1 (f32 bits)     plane 1  m2 (f32 bits)
//   plane 2  bits 0..15 the signs of q_0 .. q_{L-1} (1 = q < 0), bits 16..20 i1, bits 21..25 i2 (31 = none)
// 12 B M n_iter per word.  mag, the other-sign parity and u > 0 follow from these and the weights.
#pragma once
#include "fgnn_hip_ldpc_nms.h"
#include "ldpc_word.h"

#define NMS_MAXIT 64
#define NMS_BWD_GROUPS 512
#define NMS_PARTIAL_LDS (64 * 1024)     // the backward keeps its partial in LDS while state + partial stay within this
#define NMS_NONE 31u

struct NmsFwdParams {
    const float* llr; int64_t llr_sb;
    const int32_t *col_ptr, *row_ptr, *row_edge, *row_var;
    const float *alpha, *beta;
    uint8_t* x;
    float *post, *totals;
    int32_t *viol, *iters;
    uint32_t* record;
    int64_t B;
    int N, M, E, n_iter, share;
};

struct NmsBwdParams {
    const float *g_totals, *llr; int64_t llr_sb;
    const int32_t *col_ptr, *row_ptr, *row_edge, *row_var;
    const float *alpha, *beta;
    const uint32_t* record;
    float *g_llr, *ws;
    int64_t B;
    int N, M, E, n_iter, share, W;
};

__device__ __forceinline__ float nms_weight(const float* w, int it, int W, int share, int m, int e) {
    return w[(int64_t)(it - 1) * W + (share == 0 ? 0 : share == 1 ? m : e)];
}

// plane 0 of check m's record of word b (int64_t), iteration it (1-based); planes 1 and 2 lie M and 2 M values behind it.  (A macro:
// as an inline function the backward's address arithmetic came out in another order, and ldpc_nms.hip's code is to stay what it was.)
#define NMS_RECORD_AT(b, n_iter, it, M, m) ((((b) * (n_iter) + ((it) - 1)) * 3) * (M) + (m))

// plane 2 of a check whose row starts at r0
__device__ __forceinline__ uint32_t nms_record_pack(const LdpcMinScan& c, int r0) {
    return c.signs | (c.i1 < 0 ? NMS_NONE : (uint32_t)(c.i1 - r0)) << 16 | (c.i2 < 0 ? NMS_NONE : (uint32_t)(c.i2 - r0)) << 21;
}

static inline int64_t nms_record_bytes(int64_t B, int M, int n_iter) { return B * n_iter * 3 * (int64_t)M * 4; }
static inline int64_t nms_groups(int64_t B) { return B < 0 ? 0 : B < NMS_BWD_GROUPS ? B : NMS_BWD_GROUPS; }

static int nms_check_sizes(const char* who, int64_t B, int N, int M, int E, int n_iter, int share) {
    if (ldpc_word_check_sizes(who, N, M, E) != FGNN_OK) return FGNN_EUNSUPPORTED;
    if (B < 0 || B > 0x7fffffffll) FGNN_FAIL(FGNN_EINVAL, "%s: batch %lld outside 0 .. 2^31-1", who, (long long)B);
    if (n_iter < 1 || n_iter > NMS_MAXIT) FGNN_FAIL(FGNN_EINVAL, "%s: n_iter=%d outside 1..%d", who, n_iter, NMS_MAXIT);
    if (share < 0 || share > 2) FGNN_FAIL(FGNN_EINVAL, "%s: share=%d outside 0..2", who, share);
    return FGNN_OK;
}

// the layer tables of the layered entry points (checked for B = 0 too, the pointers for B > 0 only, like every other pointer)
static int nms_check_layers(const char* who, const int32_t* layer_ptr, const int32_t* layer_chk, int n_layers, int M, int64_t B) {
    if (n_layers < 1 || n_layers > M) FGNN_FAIL(FGNN_EINVAL, "%s: n_layers=%d outside 1..M=%d", who, n_layers, M);
    if (B > 0 && (!layer_ptr || !layer_chk)) FGNN_FAIL(FGNN_EINVAL, "%s: null layer table", who);
    return FGNN_OK;
}

// The refusals of a forward entry point, in the header's order, then the parameters.  B = 0 passes without its pointers being looked at.
static int nms_forward_args(const char* who, const float* llr, int64_t llr_sb, const int32_t* col_ptr, const int32_t* row_ptr,
                            const int32_t* row_edge, const int32_t* row_var, const float* alpha, const float* beta, int64_t B, int N,
                            int M, int E, int n_iter, int share, int stop_early, uint8_t* x, float* post, int32_t* viol, int32_t* iters,
                            float* totals, void* record, int64_t record_bytes, NmsFwdParams* p) {
    const int rc = nms_check_sizes(who, B, N, M, E, n_iter, share);
    if (rc != FGNN_OK) return rc;
    if (stop_early < 0 || stop_early > 1) FGNN_FAIL(FGNN_EINVAL, "%s: stop_early=%d outside 0..1", who, stop_early);
    if (llr_sb < 0) FGNN_FAIL(FGNN_EINVAL, "%s: negative row stride", who);
    if (stop_early && (totals || record)) FGNN_FAIL(FGNN_EINVAL, "%s: totals and record belong to the train mode (stop_early = 0)", who);
    if (B > 0) {
        if (!llr || !col_ptr || !row_ptr || !row_edge || !row_var || !alpha || !beta) FGNN_FAIL(FGNN_EINVAL, "%s: null input pointer", who);
        if (stop_early && (!x || !viol || !iters)) FGNN_FAIL(FGNN_EINVAL, "%s: null output pointer", who);
        if (!stop_early) {
            if (!totals || !record) FGNN_FAIL(FGNN_EINVAL, "%s: null totals or record in train mode", who);
            const int64_t need = nms_record_bytes(B, M, n_iter);
            if (record_bytes < need)
                FGNN_FAIL(FGNN_EINVAL, "%s: a record of %lld bytes, %lld needed", who, (long long)record_bytes, (long long)need);
        }
    }
    p->llr = llr; p->llr_sb = llr_sb;
    p->col_ptr = col_ptr; p->row_ptr = row_ptr; p->row_edge = row_edge; p->row_var = row_var;
    p->alpha = alpha; p->beta = beta;
    p->x = x; p->post = post; p->totals = totals; p->viol = viol; p->iters = iters; p->record = (uint32_t*)record;
    p->B = B; p->N = N; p->M = M; p->E = E; p->n_iter = n_iter; p->share = share;
    return FGNN_OK;
}

// ... and of a backward entry point.  B = 0: the caller ends with nms_backward_empty.
static int nms_backward_args(const char* who, const float* g_totals, const float* llr, int64_t llr_sb, const int32_t* col_ptr,
                             const int32_t* row_ptr, const int32_t* row_edge, const int32_t* row_var, const float* alpha,
                             const float* beta, const void* record, int64_t record_bytes, int64_t B, int N, int M, int E, int n_iter,
                             int share, float* g_alpha, float* g_beta, float* g_llr, void* workspace, int64_t workspace_bytes,
                             NmsBwdParams* p) {
    const int rc = nms_check_sizes(who, B, N, M, E, n_iter, share);
    if (rc != FGNN_OK) return rc;
    if (llr_sb < 0) FGNN_FAIL(FGNN_EINVAL, "%s: negative row stride", who);
    const int W = share == 0 ? 1 : share == 1 ? M : E;
    if (B > 0) {
        if (!g_totals || !col_ptr || !row_ptr || !row_edge || !row_var || !alpha || !beta || !record)
            FGNN_FAIL(FGNN_EINVAL, "%s: null input pointer", who);
        if (!g_alpha || !g_beta || !workspace) FGNN_FAIL(FGNN_EINVAL, "%s: null output or workspace pointer", who);
        if (g_llr && !llr) FGNN_FAIL(FGNN_EINVAL, "%s: g_llr needs llr (the load's clamp)", who);
        const int64_t need_rec = nms_record_bytes(B, M, n_iter);
        if (record_bytes < need_rec)
            FGNN_FAIL(FGNN_EINVAL, "%s: a record of %lld bytes, %lld needed", who, (long long)record_bytes, (long long)need_rec);
        const int64_t need_ws = nms_groups(B) * 2 * n_iter * W * 4;
        if (workspace_bytes < need_ws)
            FGNN_FAIL(FGNN_EINVAL, "%s: a workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes, (long long)need_ws);
    }
    p->g_totals = g_totals; p->llr = llr; p->llr_sb = llr_sb;
    p->col_ptr = col_ptr; p->row_ptr = row_ptr; p->row_edge = row_edge; p->row_var = row_var;
    p->alpha = alpha; p->beta = beta; p->record = (const uint32_t*)record;
    p->g_llr = g_llr; p->ws = (float*)workspace;
    p->B = B; p->N = N; p->M = M; p->E = E; p->n_iter = n_iter; p->share = share; p->W = W;
    return FGNN_OK;
}

// an empty batch's backward: zeros to g_alpha and g_beta [cnt] (null pointers: a no-op)
static int nms_backward_empty(const char* who, float* g_alpha, float* g_beta, int cnt, hipStream_t st) {
    if (g_alpha && g_beta) {
        hipError_t e = hipMemsetAsync(g_alpha, 0, 4 * (size_t)cnt, st);
        if (e == hipSuccess) e = hipMemsetAsync(g_beta, 0, 4 * (size_t)cnt, st);
        if (e != hipSuccess) FGNN_FAIL(FGNN_ELAUNCH, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    }
    return FGNN_OK;
}

// ldpc_nms.hip (internal to the library: not exported): the second launch of either backward, ldpc_nms_sum_kernel over the G
// slices of [2][cnt] floats in ``ws``
__attribute__((visibility("hidden"))) int nms_launch_sum(const char* what, const float* ws, int G, int cnt, float* g_alpha, float* g_beta, hipStream_t st);
