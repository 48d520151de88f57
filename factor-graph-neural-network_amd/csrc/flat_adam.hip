// flat_adam.hip — Adam (torch.optim.Adam's update rule, no amsgrad; the optimizer of every reference training script,
// e.g. /root/reference/train_ldpc.py:160-166) over ONE flat f32 parameter buffer in ONE pass:
//     g' = g * gscale + wd * p ;  m = b1 m + (1-b1) g' ;  v = b2 v + (1-b2) g'^2 ;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
// and, when asked, the bf16 mirror of the parameters the node-wise GEMMs read is refreshed in the same pass
// (dp.FlatAdam used eight elementwise torch kernels + one cast kernel per step).  gscale = 1 / world folds the mean of the
// all-reduced gradient into the update.  Memory-bound: 4 f32 streams read, 3 written (+ 2 B/param mirror).
//
// Gradient-norm clipping (torch.nn.utils.clip_grad_norm_(parameters, max_norm), the line in front of optimizer.step() in the
// synthetic scripts, /root/reference/train_syn_hop_factor.py:302): fgnn_grad_norm_clip reads the flat gradient once and leaves
// the norm and the clip coefficient in device memory; the *_clipped updates multiply the coefficient into gscale, one scalar
// load per thread.  No pass rewrites the gradient buffer.
#include "fgnn_common.h"
#include <math.h>

struct FaParams {
    float* p;
    const float* g;
    float* m;
    float* v;
    uint16_t* mirror;     // or NULL
    int64_t n4;           // float4 chunks
    int64_t n;            // elements (tail handled by the last thread)
    float lr_bc1, inv_sqrt_bc2, eps, b1, b2, wd, gscale;
    const float* coef;    // or NULL; {lr / bc1, 1 / sqrt(bc2)} in device memory (the capturable form: flat_adam_tick_kernel writes it)
    const float* clip;    // or NULL; the gradient-norm clip coefficient in device memory (fgnn_grad_norm_clip's out[1])
};

// The capturable step's first kernel: advance the device-resident step count and form this step's two bias-corrected
// coefficients from the device-resident learning rate, in double as the host form does.  One thread.
__global__ void flat_adam_tick_kernel(int64_t* step, const float* lr, float b1, float b2, float* coef) {
    const int64_t t = *step + 1;
    *step = t;
    const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
    coef[0] = (float)((double)*lr / bc1);
    coef[1] = (float)(1.0 / sqrt(bc2));
}

__global__ __launch_bounds__(256) void flat_adam_kernel(const FaParams a) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const float lr_bc1 = a.coef ? a.coef[0] : a.lr_bc1, inv_sqrt_bc2 = a.coef ? a.coef[1] : a.inv_sqrt_bc2;
    const float gscale = a.clip ? a.gscale * a.clip[0] : a.gscale;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n4; i += stride) {
        f32x4 p = reinterpret_cast<const f32x4*>(a.p)[i], g = reinterpret_cast<const f32x4*>(a.g)[i];
        f32x4 m = reinterpret_cast<const f32x4*>(a.m)[i], v = reinterpret_cast<const f32x4*>(a.v)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ge = fmaf(a.wd, p[e], g[e] * gscale);
            m[e] = fmaf(1.f - a.b1, ge - m[e], m[e]);                 // lerp, as torch's exp_avg.lerp_(grad, 1 - beta1)
            v[e] = fmaf(a.b2, v[e], (1.f - a.b2) * ge * ge);
            const float denom = sqrtf(v[e]) * inv_sqrt_bc2 + a.eps;
            p[e] = p[e] - lr_bc1 * (m[e] / denom);
        }
        reinterpret_cast<f32x4*>(a.p)[i] = p;
        reinterpret_cast<f32x4*>(a.m)[i] = m;
        reinterpret_cast<f32x4*>(a.v)[i] = v;
        if (a.mirror) {
            typedef __bf16 b4 __attribute__((ext_vector_type(4)));
            const b4 h = {(__bf16)p[0], (__bf16)p[1], (__bf16)p[2], (__bf16)p[3]};
            reinterpret_cast<b4*>(a.mirror)[i] = h;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int64_t j = a.n4 * 4; j < a.n; ++j) {                     // < 4 tail elements
            const float ge = fmaf(a.wd, a.p[j], a.g[j] * gscale);
            const float m = fmaf(1.f - a.b1, ge - a.m[j], a.m[j]);
            const float v = fmaf(a.b2, a.v[j], (1.f - a.b2) * ge * ge);
            a.m[j] = m; a.v[j] = v;
            const float pn = a.p[j] - lr_bc1 * (m / (sqrtf(v) * inv_sqrt_bc2 + a.eps));
            a.p[j] = pn;
            if (a.mirror) { const __bf16 h = (__bf16)pn; a.mirror[j] = __builtin_bit_cast(uint16_t, h); }
        }
    }
}

static int flat_adam_check(const float* param, const float* grad, const float* exp_avg, const float* exp_avg_sq,
                           const void* bf16_mirror, int64_t n) {
    if (!param || !grad || !exp_avg || !exp_avg_sq) FGNN_FAIL(FGNN_EINVAL, "flat_adam: null buffer");
    if (n < 0) FGNN_FAIL(FGNN_EINVAL, "flat_adam: n >= 0");
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15)
        FGNN_FAIL(FGNN_EINVAL, "flat_adam: buffers must be 16-byte aligned");
    if (bf16_mirror && ((uintptr_t)bf16_mirror & 7)) FGNN_FAIL(FGNN_EINVAL, "flat_adam: mirror must be 8-byte aligned");
    return FGNN_OK;
}

static int flat_adam_launch(FaParams& a, hipStream_t stream) {
    int64_t g = (a.n4 + 255) / 256;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return fgnn_launch("flat_adam", flat_adam_kernel, dim3((unsigned)g), dim3(256), 0, stream, a);
}

// step = 1-based step count (bias corrections 1 - beta^step are formed in double on the host)
static int flat_adam_host(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_mirror,
                          int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                          float grad_scale, int64_t step, const float* clip, fgnn_stream_t stream) {
    if (int rc = flat_adam_check(param, grad, exp_avg, exp_avg_sq, bf16_mirror, n)) return rc;
    if (step < 1) FGNN_FAIL(FGNN_EINVAL, "flat_adam: step >= 1");
    if (n == 0) return FGNN_OK;
    FaParams a;
    a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.mirror = (uint16_t*)bf16_mirror;
    a.n = n; a.n4 = n / 4; a.coef = nullptr; a.clip = clip;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    a.lr_bc1 = (float)((double)lr / bc1);
    a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    a.eps = eps; a.b1 = beta1; a.b2 = beta2; a.wd = weight_decay; a.gscale = grad_scale;
    return flat_adam_launch(a, fgnn_stream(stream));
}

// The same update with NOTHING step-dependent in the launch arguments, so that the launch can be recorded into a hipGraph and
// replayed: the step count (*step_dev, int64, starts at 0, advanced by one per call) and the learning rate (*lr_dev, f32; a
// scheduler overwrites it between replays) live in device memory; coef_dev is two floats of scratch.  Two launches.
static int flat_adam_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_mirror,
                         int64_t n, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                         float grad_scale, int64_t* step_dev, float* coef_dev, const float* clip, fgnn_stream_t stream) {
    if (int rc = flat_adam_check(param, grad, exp_avg, exp_avg_sq, bf16_mirror, n)) return rc;
    if (!lr_dev || !step_dev || !coef_dev) FGNN_FAIL(FGNN_EINVAL, "flat_adam_dev: null lr / step / coefficient buffer");
    if (int rc = fgnn_launch("flat_adam_tick", flat_adam_tick_kernel, dim3(1), dim3(1), 0, fgnn_stream(stream), step_dev, lr_dev, beta1, beta2, coef_dev)) return rc;
    if (n == 0) return FGNN_OK;
    FaParams a;
    a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.mirror = (uint16_t*)bf16_mirror;
    a.n = n; a.n4 = n / 4; a.coef = coef_dev; a.lr_bc1 = 0.f; a.inv_sqrt_bc2 = 0.f; a.clip = clip;
    a.eps = eps; a.b1 = beta1; a.b2 = beta2; a.wd = weight_decay; a.gscale = grad_scale;
    return flat_adam_launch(a, fgnn_stream(stream));
}

extern "C" int fgnn_flat_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_mirror,
                              int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                              float grad_scale, int64_t step, fgnn_stream_t stream) {
    return flat_adam_host(param, grad, exp_avg, exp_avg_sq, bf16_mirror, n, lr, beta1, beta2, eps, weight_decay, grad_scale, step,
                          nullptr, stream);
}

extern "C" int fgnn_flat_adam_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_mirror,
                                  int64_t n, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                  float grad_scale, int64_t* step_dev, float* coef_dev, fgnn_stream_t stream) {
    return flat_adam_dev(param, grad, exp_avg, exp_avg_sq, bf16_mirror, n, lr_dev, beta1, beta2, eps, weight_decay, grad_scale,
                         step_dev, coef_dev, nullptr, stream);
}

// The two updates with g' = g * grad_scale * (*clip_dev) + wd * p: clip_dev is fgnn_grad_norm_clip's out + 1 (or any f32 in device
// memory).  The product grad_scale * (*clip_dev) is formed once per thread in f32: a coefficient of 1 gives the unclipped entry
// point's bits, a coefficient c those of the unclipped entry point called with the f32 product grad_scale * c.
extern "C" int fgnn_flat_adam_clipped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_mirror,
                                      int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                                      float grad_scale, int64_t step, const float* clip_dev, fgnn_stream_t stream) {
    if (!clip_dev) FGNN_FAIL(FGNN_EINVAL, "flat_adam_clipped: null clip coefficient");
    return flat_adam_host(param, grad, exp_avg, exp_avg_sq, bf16_mirror, n, lr, beta1, beta2, eps, weight_decay, grad_scale, step,
                          clip_dev, stream);
}

extern "C" int fgnn_flat_adam_dev_clipped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_mirror,
                                          int64_t n, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                          float grad_scale, int64_t* step_dev, float* coef_dev, const float* clip_dev,
                                          fgnn_stream_t stream) {
    if (!clip_dev) FGNN_FAIL(FGNN_EINVAL, "flat_adam_dev_clipped: null clip coefficient");
    return flat_adam_dev(param, grad, exp_avg, exp_avg_sq, bf16_mirror, n, lr_dev, beta1, beta2, eps, weight_decay, grad_scale,
                         step_dev, coef_dev, clip_dev, stream);
}

// ---- the gradient's norm and torch.nn.utils.clip_grad_norm_'s coefficient ----------------------------------------------------------
// Stage 1: workgroup w sums the squares of its grid-stride share of the float4 chunks in f64 (a thread its chunks in order, a wave
// by an xor butterfly, the four waves in order) -> part[w]; workgroup 0's first thread adds the < 4 tail elements to its own sum
// first.  Stage 2 (one thread) adds the partials in workgroup order.  The grid depends on n alone: bit-reproducible, and nothing
// in the launch arguments depends on the step, so both launches can be recorded into a hipGraph.
#define GN_MAXGRID 256

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n4, int64_t n, double* __restrict__ part) {
    __shared__ double s_sum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t j = n4 * 4; j < n; ++j) acc += (double)g[j] * (double)g[j];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += (double)v[e] * (double)v[e];
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
    if (lane == 0) s_sum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
}

// out[0] = sqrt(sum) * grad_scale (f64, rounded once); out[1] = min(1, max_norm / (out[0] + 1e-6)) in f32 as torch forms it
// (torch.clamp(max=1) keeps a NaN; an infinite norm gives 0, and 0 * inf = NaN in the update, as torch's in-place scaling gives)
__global__ void grad_norm_final_kernel(const double* __restrict__ part, int npart, float max_norm, float grad_scale,
                                       float* __restrict__ out) {
    double s = 0.0;
    for (int i = 0; i < npart; ++i) s += part[i];
    const float norm = (float)(sqrt(s) * (double)grad_scale);
    const float c = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = c > 1.f ? 1.f : c;
}

extern "C" int64_t fgnn_grad_norm_clip_workspace_bytes(void) { return (int64_t)GN_MAXGRID * sizeof(double); }

extern "C" int fgnn_grad_norm_clip(const float* grad, int64_t n, float max_norm, float grad_scale, float* out, void* workspace,
                                   int64_t workspace_bytes, fgnn_stream_t stream) {
    if (!grad || !out) FGNN_FAIL(FGNN_EINVAL, "grad_norm_clip: null pointer");
    if (n < 0) FGNN_FAIL(FGNN_EINVAL, "grad_norm_clip: n >= 0");
    if ((uintptr_t)grad & 15) FGNN_FAIL(FGNN_EINVAL, "grad_norm_clip: the gradient must be 16-byte aligned");
    if (!workspace || workspace_bytes < fgnn_grad_norm_clip_workspace_bytes() || ((uintptr_t)workspace & 7))
        FGNN_FAIL(FGNN_EINVAL, "grad_norm_clip: an 8-byte aligned workspace of fgnn_grad_norm_clip_workspace_bytes() bytes needed");
    hipStream_t st = fgnn_stream(stream);
    double* part = (double*)workspace;
    const int64_t n4 = n / 4;
    int64_t g = (n4 + 4 * 256 - 1) / (4 * 256);          // ~4 chunks per thread
    if (g > GN_MAXGRID) g = GN_MAXGRID;
    if (g < 1) g = 1;
    if (n > 0) {
        if (int rc = fgnn_launch("grad_norm_clip", grad_sumsq_kernel, dim3((unsigned)g), dim3(256), 0, st, grad, n4, n, part)) return rc;
    }
    return fgnn_launch("grad_norm_clip", grad_norm_final_kernel, dim3(1), dim3(1), 0, st, part, n > 0 ? (int)g : 0, max_norm, grad_scale, out);
}
