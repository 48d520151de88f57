// Shared device/host helpers for the FGNN gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "fgnn_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define FGNN_THREADS 256
#define FGNN_WAVES 4

// ---- storage-type helpers: kernels compute in f32, store f32 or bf16 ------------------
struct bf16_t { uint16_t v; };

__device__ __forceinline__ float fgnn_ld(const float* p) { return *p; }
__device__ __forceinline__ float fgnn_ld(const bf16_t* p) {
    return __uint_as_float(((uint32_t)p->v) << 16);
}
__device__ __forceinline__ void fgnn_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void fgnn_st(bf16_t* p, float v) {
    // native fptrunc: v_cvt_pk_bf16_f32 on gfx950 (round-to-nearest-even, NaN preserved)
    const __bf16 h = (__bf16)v;
    p->v = __builtin_bit_cast(uint16_t, h);
}

// four consecutive elements (16-B / 8-B aligned)
__device__ __forceinline__ void fgnn_st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void fgnn_st4(bf16_t* p, f32x4 v) {
    typedef __bf16 bf16x4_n __attribute__((ext_vector_type(4)));
    const bf16x4_n h = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    *reinterpret_cast<bf16x4_n*>(p) = h;
}
__device__ __forceinline__ f32x4 fgnn_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 fgnn_ld4(const bf16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return (f32x4){__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                   __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
}

// ---- host-side error plumbing ---------------------------------------------------------
void fgnn_set_error(const char* fmt, ...);
void fgnn_note_kernel(const char* fmt, ...);   // records which kernel a dispatch chose (fgnn_last_kernel)
#define FGNN_FAIL(code, ...) do { fgnn_set_error(__VA_ARGS__); return (code); } while (0)
// a kernel family's plan turns a call down (returns 0); FGNN_TRACE=1 prints which rule
int fgnn_reject(const char* family, int rule);
#define FGNN_REJECT(family, rule) return fgnn_reject(family, rule)

// phase-timeline stamps (tuning aid, -DFGNN_ENABLE_PROF builds, read with FGNN_PROF=1): fgnn_prof_begin gives the launch a zeroed
// device buffer of 256 stamps (NULL when off), fgnn_prof_print waits for the launch and prints rows x cols stamps from slot `first`
// on (row stride `stride`) relative to that slot.  The product build has neither.
#ifdef FGNN_ENABLE_PROF
long long* fgnn_prof_begin();
void fgnn_prof_print(const long long* prof, const char* tag, int first, int rows, int cols, int stride);
#else
static inline long long* fgnn_prof_begin() { return nullptr; }
static inline void fgnn_prof_print(const long long*, const char*, int, int, int, int) {}
#endif

static inline int fgnn_round_up(int v, int m) { return (v + m - 1) / m * m; }

#include "fgnn_launch.h"   // every kernel launch and its error report

// ---- host helpers shared by the translation units (not C ABI) ---------------------------
// The launching ones return FGNN_OK or FGNN_ELAUNCH with the message already set (fgnn_launch.h): callers pass the code up.
// mpconv_bwd_res.hip: fold nslab slabs (slab_len apart) of [nw weights + bias] floats into gW / gbias in a fixed order; _ld: the
// slab's [nw / ncols][ncols] weight block lands in rows `ld` apart (a column block of a wider gW)
int fgnn_launch_slab_reduce(const float* ws, int nslab, int64_t slab_len, int64_t nw, float* gW, float* gbias, hipStream_t st);
int fgnn_launch_slab_reduce_ld(const float* ws, int nslab, int64_t slab_len, int64_t nw, int ncols, int ld, float* gW,
                               float* gbias, hipStream_t st);
// the same fold, STORED (out[i] = sum over the slabs): for outputs that are not accumulators
int fgnn_launch_slab_store(const float* ws, int nslab, int64_t slab_len, float* out, hipStream_t st);
// fold_batch.hip: called instead of launching a slab fold: true = recorded (deferral is on), false = launch it yourself
bool fgnn_fold_push(const float* ws, int nslab, int64_t slab_len, int64_t nw, float* gW, float* gb, int kind, int a, int b, int c, int d);
// bnact.hip: the stand-alone BatchNorm finalisers and the bf16 backward sums
int fgnn_bn_finalize_launch(const float* partials, int npartials, int C, const fgnn_bn_final* fin, hipStream_t st);
int fgnn_bn_bwd_final_raw_launch(const float* partials, int npartials, int C, const float* mean, const float* invstd, float* dsum,
                                 float* gweight, float* gbias, hipStream_t st);
int fgnn_bn_backward_sums_bf16(const void* x, const void* gy, int64_t R, int C, const float* mean, const float* invstd,
                               const float* gamma, const float* beta, float slope, float* gweight, float* gbias,
                               void* workspace, void* fold_scratch, hipStream_t st, const float** dsum_out);
