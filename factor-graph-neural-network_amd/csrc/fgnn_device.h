// Device primitives shared by the gfx950 kernels: one definition of each, so a fix reaches every caller.
#pragma once
#include "fgnn_common.h"

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));      // one bf16 MFMA operand fragment (8 k values of a lane)
typedef short s16x4 __attribute__((ext_vector_type(4)));         // the ds_read_b64_tr_b16 result and the 16x16x16 bf16 MFMA operand

// two f32 -> one dword of bf16 (a low, b high), round-to-nearest-even.  Native fptrunc -> one v_cvt_pk_bf16_f32.  NOT inline
// asm: an asm statement reading MFMA results directly gets none of the compiler's MFMA->VALU wait states (observed: one node
// tile of stale P values once the accumulators stopped living in AGPRs).
__device__ __forceinline__ unsigned fgnn_pack2(float a, float b) {
    const bf16x2 h = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned, h);
}
// the low / high bf16 of a dword, as f32
__device__ __forceinline__ float fgnn_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float fgnn_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
// 8 consecutive f32 (16-byte aligned) -> one fragment
__device__ __forceinline__ bf16x8 fgnn_frag8(const float* p8) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p8), b = *reinterpret_cast<const f32x4*>(p8 + 4);
    return __builtin_bit_cast(bf16x8, make_uint4(fgnn_pack2(a[0], a[1]), fgnn_pack2(a[2], a[3]),
                                                 fgnn_pack2(b[0], b[1]), fgnn_pack2(b[2], b[3])));
}

// uniform 64-bit base + UNSIGNED 32-bit per-lane byte offset: the form that compiles to `global_load v, v_off, s[base]`.  A
// signed or 64-bit per-lane offset becomes a per-lane 64-bit pointer (two VGPRs), hoisted out of the sample loop and SPILLED in
// the kernels that run at 256 VGPRs — and a spill reload is a memory operation that waits (vmcnt(0)) for every load issued
// before it: the layer kernel's next-sample prefetch then paid two or three HBM round trips back to back, ~3 000 cycles per
// sample (profiles/r06/infer_layer_phase_timeline.txt, phase 7 -> 8).
template <typename T> __device__ __forceinline__ const T* fgnn_at(const void* base, unsigned byte_off) {
    return reinterpret_cast<const T*>(static_cast<const char*>(base) + byte_off);
}
template <typename T> __device__ __forceinline__ T* fgnn_at(void* base, unsigned byte_off) {
    return reinterpret_cast<T*>(static_cast<char*>(base) + byte_off);
}

// One LDS-DMA piece: 64 lanes x 16 bytes of global memory, lane l's bytes land at lds_dst + 16 l, no registers in between
// (tools/ubench/lds_dma_tr.hip).  M0 is compiler-reserved: saved and restored inside the statement (cdna_hip_programming.md
// §5.7).  The compiler's s_waitcnt bookkeeping does not count these loads: wait for them with fgnn_wait_vm<>.
__device__ __forceinline__ void fgnn_dma16(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// the same with a UNIFORM 64-bit base (scalar registers) + an unsigned 32-bit per-lane byte offset: no 64-bit per-lane address
// to carry across a loop (see fgnn_at)
__device__ __forceinline__ void fgnn_dma16s(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
// s_waitcnt vmcnt(N): at most N of this wave's vector-memory loads (LDS-DMA pieces included) still outstanding
template <int N> __device__ __forceinline__ void fgnn_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ds_read_b64_tr_b16: the 16 lanes of a group each name 4 consecutive bf16 of a [4 keys][16 columns] block (lane i: key i >> 2,
// columns 4 (i & 3) ..), lane c of the group receives column c of the four keys (tools/ubench/lds_dma_tr.hip)
__device__ __forceinline__ uint2 fgnn_tr16(unsigned lds_addr) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_s16x4*>(static_cast<uintptr_t>(lds_addr)));
    return __builtin_bit_cast(uint2, v);
}

// rows r0..r7 each hold columns (c0 c1 | c2 c3) as two dwords: gather column P's eight values (one fragment's worth)
template <int P>
__device__ __forceinline__ uint4 fgnn_perm_col(const uint2 (&r)[8]) {
    constexpr unsigned sel = (P & 1) ? 0x07060302u : 0x05040100u;     // high / low halves of (hi:b, lo:a)
    unsigned w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned a = P < 2 ? r[2 * q].x : r[2 * q].y, b = P < 2 ? r[2 * q + 1].x : r[2 * q + 1].y;
        w[q] = __builtin_amdgcn_perm(b, a, sel);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ uint4 fgnn_perm_col_dyn(const uint2 (&r)[8], int P) {
    switch (P) {
        case 0: return fgnn_perm_col<0>(r);
        case 1: return fgnn_perm_col<1>(r);
        case 2: return fgnn_perm_col<2>(r);
        default: return fgnn_perm_col<3>(r);
    }
}

// sum / max over the 16 lanes of a DPP row, in every lane of the row (a fixed tree: quad, then the row by mirrors)
__device__ __forceinline__ float fgnn_row_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));   // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));   // row_mirror
    return v;
}
__device__ __forceinline__ float fgnn_row_max(float v) {
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0xB1, 0xF, 0xF, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x4E, 0xF, 0xF, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x141, 0xF, 0xF, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x140, 0xF, 0xF, false)));
    return v;
}
// lane `lane`'s v, in every lane
__device__ __forceinline__ float fgnn_bcast(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
// acc + p.lo e.lo + p.hi e.hi, p and e packed bf16 pairs
__device__ __forceinline__ float fgnn_dot2(unsigned p, unsigned e, float acc) {
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, p), __builtin_bit_cast(bf16x2, e), acc, false);
}

// ---- the synthetic-PGM labelling head (pgm_eval.hip, pgm_loss.hip): one read and one decision rule for both ----
// the two logits of one variable, o = b * sb + i * vs its class-0 element and cs the class stride; DK = FGNN_PGM_DEC_F32 / _BF16
template <int DK> __device__ __forceinline__ void fgnn_pgm_logits(const void* dec, int64_t o, int64_t cs, float& v0, float& v1) {
    if (DK == FGNN_PGM_DEC_F32) {
        const float* d = static_cast<const float*>(dec);
        v0 = d[o]; v1 = d[o + cs];
    } else {
        const bf16_t* d = static_cast<const bf16_t*>(dec);
        v0 = fgnn_ld(d + o); v1 = fgnn_ld(d + o + cs);
    }
}
// variable i's label of sample b (int64, variables contiguous, sb between samples)
__device__ __forceinline__ int64_t fgnn_pgm_label(const int64_t* label, int64_t b, int64_t sb, int i) { return label[b * sb + i]; }
// torch.argmax over (v0, v1): the first maximum, NaN above everything (a NaN v0 keeps 0)
__device__ __forceinline__ int fgnn_pgm_decide(float v0, float v1) {
    return v1 > v0 || (__builtin_isnan(v1) && !__builtin_isnan(v0));
}
