// mpconv_bwd_hyper.hip — backward of the VF/FV message operator for the two "hyper-edge" calls of a
// factor graph with one factor that touches every variable (the LDPC hyper-factor of
// /root/reference/train_ldpc.py:60-75: V->F with M = 1 destination of degree k = 96, F->V with N = 1 source
// feeding M = 96 destinations through k = 1 edges), single edge type, max aggregator, NO_EXTENSION, and a
// CONSTANT etype (getype == NULL).  Same maths as mpconv_bwd_res.hip (autograd through
// /root/reference/lib/model/mpnn/mp_nn.py:115-175) but neither call is GEMM-shaped once the routing is known:
//
//  fan-in  (M == 1):  z[o] = max_j et[j] * P[idx[j], o].  Only ONE neighbour per output channel carries
//      gradient, so dP has nou non-zeros out of N*nou:
//          c_o = et[j*_o] * gz[o],  n*_o = idx[j*_o]
//          dx[n, :]  = sum_{o : n*_o = n} c_o * W[:, o]          (all other rows are zero)
//          dW[:, o] += c_o * x[n*_o, :]
//      = 2 * nin * nou MACs per sample instead of the dense 3 * N * nin * nou.
//  fan-out (N == 1, k == 1):  z[m, o] = et[m] * P[0, o]:
//          dP[o] = sum_m et[m] * gz[m, o],  dx = W dP,  dW += x (x) dP
//      = one weighted column sum of gz plus two matrix-vector products.
//
// Schedule of both: ONE WAVE PER SAMPLE (8 waves per workgroup, samples interleaved over all waves of the grid), W^T resident
// in LDS, dW accumulated in registers over all samples of a wave, folded across the 8 waves through LDS in a fixed order
// (bit-reproducible) and written to the workgroup's slab of the caller's workspace (summed by the slab reduce of
// mpconv_bwd_res.hip).
//  fan-out: lane <-> input channel for the W-shaped work (row o of W^T contiguous over c: conflict-free), dP broadcast with
//      v_readlane, the fold in eight turns (bh_flush).
//  fan-in:  lane <-> output channel for the routing and for dW (each lane reads its own winner's row in 16-byte pieces),
//      lane <-> (row, 8 input channels) for dx (per-row winner masks in LDS, one 16-byte store per lane, untouched rows
//      written as zeros by the same stores), the fold in one pass (two in the wide instances), in wave order; see the kernel.  What it moves is the dense, mostly
//      zero gx; measured phases and rates: profiles/fanin_bwd/README.md.
#include "fgnn_common.h"
#include "fgnn_device.h"
#include "mpconv_dispatch.h"
#include <stdlib.h>

#define BH_THREADS 512
#define BH_WAVES 8
#define BH_ROWS 128      // fan-in: node rows per dx pass (their winner masks are in LDS)

struct BhParams {
    fgnn_mpconv_desc d;
    const void* x;
    const int64_t* idx;
    const void* et;
    const float* W;
    const void* gz;
    const uint8_t* argmax;
    void* gx;
    float* ws;           // per-workgroup slabs [grid][nin*nou + nou]
    int has_bias;
    int wvec;            // fan-in: W is 16-byte aligned
    long long* prof;     // FGNN_PROF (builds with -DFGNN_ENABLE_PROF only): phase timeline of the fan-in kernel
};

extern __shared__ __attribute__((aligned(16))) float fgnn_lds_bh[];


// Stage W [nin][nou] (row-major) transposed into LDS: Wl[o * nin + c].
template <int NIN, int NOU>
__device__ __forceinline__ void bh_stage_w(const float* __restrict__ W, float* Wl, int tid) {
    for (int f = tid; f < NIN * NOU; f += BH_THREADS) {
        const int c = f / NOU, o = f - c * NOU;
        Wl[o * NIN + c] = W[f];
    }
}

// Fold the per-wave dW / dbias accumulators across the workgroup's waves (fixed order) and write the slab.
// dW[i][o] belongs to (c = lane + 64 i, o); gb_val is this lane's dbias for channel gb_ch (or gb_ch < 0).
template <int NI, int NO>
__device__ __forceinline__ void bh_flush(const BhParams& p, float* Wl, float* bl, float (&dW)[NI][64 * NO],
                                         const float (&gbv)[4 * NO], const int (&gbc)[4 * NO], int ngb, int tid,
                                         int lane, int wave) {
    constexpr int NIN = 64 * NI, NOU = 64 * NO;
    __syncthreads();                                   // every wave is done with W^T: the buffer becomes the fold
    for (int w = 0; w < BH_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int o = 0; o < NOU; ++o) {
                    float* q = Wl + o * NIN + lane + 64 * i;
                    *q = (w == 0) ? dW[i][o] : *q + dW[i][o];
                }
#pragma unroll
            for (int t = 0; t < 4 * NO; ++t)
                if (t < ngb && gbc[t] >= 0) bl[gbc[t]] = (w == 0) ? gbv[t] : bl[gbc[t]] + gbv[t];
        }
        __syncthreads();
    }
    float* slab = p.ws + (int64_t)blockIdx.x * (NIN * NOU + NOU);
    for (int f = tid; f < NIN * NOU; f += BH_THREADS) {
        const int c = f / NOU, o = f - c * NOU;
        slab[f] = Wl[o * NIN + c];
    }
    for (int f = tid; f < NOU; f += BH_THREADS) slab[NIN * NOU + f] = bl[f];
}

// ----------------------------------------------------------------------------------------
// fan-in: M == 1, net == 1
// ----------------------------------------------------------------------------------------
// phase stamps (tuning aid, -DFGNN_ENABLE_PROF builds read with FGNN_PROF=1): workgroup 0, every wave: 0 start, 1 W^T staged,
// then for the wave's first sample 2 routing known, 3 dx written, 4 dW accumulated, 5 all samples done, 6 first fold pass done, 7 slab written.
// Each stamp first waits for the wave's outstanding memory operations, so a phase is charged what it issued.
#ifdef FGNN_ENABLE_PROF
#define BH_STAMP(slot) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); if (p.prof && blockIdx.x == 0 && lane == 0) p.prof[wave * 16 + (slot)] = __builtin_readcyclecounter(); } while (0)
#else
#define BH_STAMP(slot) do { } while (0)
#endif

// 8 consecutive channels at p as f32 / from f32.  PK: channel stride 1 and p 16-byte aligned (one or two 16-byte accesses),
// otherwise element by element, `sc` apart.
template <bool PK> __device__ __forceinline__ void bh_unpack8(const uint4 u, float (&v)[8]) {
    v[0] = fgnn_lo(u.x); v[1] = fgnn_hi(u.x); v[2] = fgnn_lo(u.y); v[3] = fgnn_hi(u.y);
    v[4] = fgnn_lo(u.z); v[5] = fgnn_hi(u.z); v[6] = fgnn_lo(u.w); v[7] = fgnn_hi(u.w);
}
template <bool PK> __device__ __forceinline__ void bh_ld8(const bf16_t* p, int64_t sc, float (&v)[8]) {
    if (PK) {
        bh_unpack8<PK>(*reinterpret_cast<const uint4*>(p), v);
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = fgnn_ld(p + u * sc);
    }
}
template <bool PK> __device__ __forceinline__ void bh_ld8(const float* p, int64_t sc, float (&v)[8]) {
    if (PK) {
        const f32x4 a = fgnn_ld4(p), b = fgnn_ld4(p + 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) { v[u] = a[u]; v[4 + u] = b[u]; }
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[u * sc];
    }
}
template <bool PK> __device__ __forceinline__ void bh_st8(bf16_t* p, int64_t sc, const float (&v)[8]) {
    if (PK) {
        *reinterpret_cast<uint4*>(p) = make_uint4(fgnn_pack2(v[0], v[1]), fgnn_pack2(v[2], v[3]), fgnn_pack2(v[4], v[5]), fgnn_pack2(v[6], v[7]));
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) fgnn_st(p + u * sc, v[u]);
    }
}
template <bool PK> __device__ __forceinline__ void bh_st8(float* p, int64_t sc, const float (&v)[8]) {
    if (PK) {
        fgnn_st4(p, (f32x4){v[0], v[1], v[2], v[3]});
        fgnn_st4(p + 4, (f32x4){v[4], v[5], v[6], v[7]});
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u * sc] = v[u];
    }
}

// Routing of sample b, lane <-> output channel (lane + 64 q), in two dependent reads: (a) the upstream gradient and the winner
// slot, (b) the slot's source node and edge weight; bh_route_done turns them into (n*_o, c_o = et[j*_o] gz[o]).  The reads only
// LOAD (nothing is computed from a value in the block that fetched it), so that the caller chooses where each is waited for.
template <typename T, int NO>
__device__ __forceinline__ void bh_route_a(const BhParams& p, int b, int lane, T (&graw)[NO], uint8_t (&jraw)[NO]) {
    const fgnn_mpconv_desc& d = p.d;
#pragma unroll
    for (int q = 0; q < NO; ++q) {
        const int64_t yo = (int64_t)b * d.y_sb + (int64_t)(lane + 64 * q) * d.y_sc;
        graw[q] = reinterpret_cast<const T*>(p.gz)[yo];
        jraw[q] = p.argmax[yo];
    }
}
template <typename T, int NO>
__device__ __forceinline__ void bh_route_b(const BhParams& p, int b, const uint8_t (&jraw)[NO], int (&nraw)[NO], T (&eraw)[NO]) {
    const fgnn_mpconv_desc& d = p.d;
#pragma unroll
    for (int q = 0; q < NO; ++q) {
        const int js = jraw[q] < d.k ? jraw[q] : d.k - 1;
        // (the low half of the int64 id: all the clamp below looks at; a 64-bit destination's unused half gets reused while the
        // load is in flight, and the reuse waits for the load)
        nraw[q] = reinterpret_cast<const int*>(p.idx)[2 * ((int64_t)b * d.idx_sb + (int64_t)js * d.idx_sk)];
        eraw[q] = reinterpret_cast<const T*>(p.et)[(int64_t)b * d.et_sb + (int64_t)js * d.et_sk];
    }
}
template <typename T, int NO>
__device__ __forceinline__ void bh_route_done(const BhParams& p, const T (&graw)[NO], const int (&nraw)[NO], const T (&eraw)[NO],
                                              float (&g)[NO], int (&ns)[NO], float (&cf)[NO]) {
#pragma unroll
    for (int q = 0; q < NO; ++q) {
        const int n = nraw[q];
        ns[q] = n < 0 ? 0 : (n >= p.d.N ? p.d.N - 1 : n);
        g[q] = fgnn_ld(&graw[q]);
        cf[q] = g[q] * fgnn_ld(&eraw[q]);
    }
}

// this wave's LDS writes are visible to its own later reads (one wave: LDS operations complete in order; the statement keeps the
// compiler from moving any across it)
__device__ __forceinline__ void bh_wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// LDS of the fan-in kernel (bytes).  Sample loop: W^T [NOU][NIN + 4] f32, then per wave the winner masks of BH_ROWS node rows
// (one 64-bit word per row and 64 output channels) and the NOU routed coefficients.  Afterwards the same memory is the fold:
// eight regions of [NIN / (NI NO)][NOU] + [NOU] f32.
static __host__ __device__ constexpr int bh_fanin_wt_bytes(int NI, int NO) { return 64 * NO * (64 * NI + 4) * 4; }
static __host__ __device__ constexpr int bh_fanin_lds(int NI, int NO) {
    const int loop = bh_fanin_wt_bytes(NI, NO) + BH_WAVES * (NO * BH_ROWS * 8 + 64 * NO * 4);
    const int fold = BH_WAVES * (64 * NI * 64 * NO / (NI * NO) + 64 * NO) * 4;
    return loop > fold ? loop : fold;
}

// One wave per sample.  PK: x / gx are channel-fastest with 16-byte aligned rows (the layout of the training step); otherwise the
// same schedule with element accesses.
//   routing  lane <-> output channel o: (n*_o, c_o), read one and two samples ahead.
//   dx       lane o ORs bit o into the LDS mask of row n*_o.  Then RG = 512 / NIN rows at a time, lane <-> (row, 8 input
//            channels): the row's winners in ASCENDING channel order, acc = fma(c_o, W[c, o], acc) from 0 — the sum and its order
//            are those of a lane-per-channel loop over o — and one 16-byte store per lane; a row without winners stores its
//            zeros the same way.  Every gx element is written exactly once.
//   dW       lane o reads its winner's row x[n*_o, :] in 16-byte pieces and accumulates dW[:, o] in its own registers (bf16: the
//            pieces are fetched before the dx phase and consumed after it).
//   tail     the eight waves' registers go to LDS once; every wave adds an eighth of the rows in wave order and writes them to
//            the [nin][nou] slab, lane <-> o: 256-byte rows.
template <typename T, int NI, int NO, bool PK>
__global__ __launch_bounds__(BH_THREADS) void mpconv_bwd_fanin_kernel(const BhParams p) {
    constexpr int NIN = 64 * NI, NOU = 64 * NO, LD = NIN + 4;
    constexpr int CPR = NIN / 8, RG = 64 / CPR;            // 8-channel chunks per row; rows per wave-wide access
    constexpr bool PRE = PK && sizeof(T) == 2;             // winner rows fetched ahead of the dx phase
    const fgnn_mpconv_desc& d = p.d;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* Wl = fgnn_lds_bh;                               // [NOU][LD]
    unsigned long long* mk = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(fgnn_lds_bh) + bh_fanin_wt_bytes(NI, NO))
                             + wave * (NO * BH_ROWS);      // [BH_ROWS][NO]
    float* cfl = reinterpret_cast<float*>(reinterpret_cast<char*>(fgnn_lds_bh) + bh_fanin_wt_bytes(NI, NO) + BH_WAVES * NO * BH_ROWS * 8)
                 + wave * NOU;                             // [NOU]
    BH_STAMP(0);

    const T* X = reinterpret_cast<const T*>(p.x);
    T* GX = reinterpret_cast<T*>(p.gx);
    const int N = d.N;
    const int nwaves = gridDim.x * BH_WAVES;
    int b = blockIdx.x * BH_WAVES + wave;

    // The routing runs ahead of the work: while sample b is worked on, read (b) of the wave's next sample and read (a) of the one
    // after it are in flight.  (vmcnt counts loads and stores in one order, so a value loaded before the gx stores and used after
    // them waits for the stores too: everything a sample needs from memory is asked for before its first store.)  Idle waves
    // and the reads past a wave's last sample name a sample that exists, and what they return is dropped.
    const auto sample = [&](int s) { return s < d.B ? s : d.B - 1; };
    T graw[NO], eraw[NO], graw2[NO];
    uint8_t jraw[NO], jraw2[NO];
    int nraw[NO];
    bh_route_a<T, NO>(p, sample(b), lane, graw, jraw);
    // W [nin][nou] -> W^T: thread <-> (input channel c, four output channels); the LDS writes of a wave fall in consecutive banks
    constexpr int WQ = NIN * NOU / 4 / BH_THREADS;         // 16-byte pieces per thread
    if (p.wvec) {
        f32x4 w[WQ];
#pragma unroll
        for (int t = 0; t < WQ; ++t) {
            const int f = tid + t * BH_THREADS;
            w[t] = *reinterpret_cast<const f32x4*>(p.W + (f % NIN) * NOU + (f / NIN) * 4);
        }
        bh_route_b<T, NO>(p, sample(b), jraw, nraw, eraw);
        bh_route_a<T, NO>(p, sample(b + nwaves), lane, graw2, jraw2);
#pragma unroll
        for (int t = 0; t < WQ; ++t) {
            const int f = tid + t * BH_THREADS;
#pragma unroll
            for (int u = 0; u < 4; ++u) Wl[((f / NIN) * 4 + u) * LD + f % NIN] = w[t][u];
        }
    } else {
        bh_route_b<T, NO>(p, sample(b), jraw, nraw, eraw);
        bh_route_a<T, NO>(p, sample(b + nwaves), lane, graw2, jraw2);
        for (int f = tid; f < NIN * NOU; f += BH_THREADS) {
            const int c = f % NIN, o = f / NIN;
            Wl[o * LD + c] = p.W[c * NOU + o];
        }
    }
    float g[NO], cf[NO];
    int ns[NO];
    bh_route_done<T, NO>(p, graw, nraw, eraw, g, ns, cf);
#pragma unroll
    for (int q = 0; q < NO; ++q) { graw[q] = graw2[q]; jraw[q] = jraw2[q]; }
    __syncthreads();
    BH_STAMP(1);

    float dW[NO][NIN];                                     // dW[q][c]: input channel c, output channel lane + 64 q
#pragma unroll
    for (int q = 0; q < NO; ++q)
#pragma unroll
        for (int c = 0; c < NIN; ++c) dW[q][c] = 0.f;
    float gbv[NO];
#pragma unroll
    for (int q = 0; q < NO; ++q) gbv[q] = 0.f;
#ifdef FGNN_ENABLE_PROF
    bool first = true;
#endif

    while (b < d.B) {
        const int nb = b + nwaves;
        const T* xb = X + (int64_t)b * d.x_sb;
        T* gxb = GX + (int64_t)b * d.x_sb;
#pragma unroll
        for (int q = 0; q < NO; ++q) gbv[q] += g[q];
#ifdef FGNN_ENABLE_PROF
        if (first) BH_STAMP(2);
#endif
        bh_route_b<T, NO>(p, sample(nb), jraw, nraw, eraw);
        uint4 xraw[PRE ? NO : 1][PRE ? CPR : 1];
        if constexpr (PRE) {
#pragma unroll
            for (int q = 0; q < NO; ++q)
#pragma unroll
                for (int i = 0; i < CPR; ++i)
                    xraw[q][i] = *reinterpret_cast<const uint4*>(xb + (int64_t)ns[q] * d.x_sn + 8 * i);
        }
        bh_route_a<T, NO>(p, sample(nb + nwaves), lane, graw2, jraw2);

        // ---- dx ----
#pragma unroll
        for (int q = 0; q < NO; ++q) cfl[lane + 64 * q] = cf[q];
        for (int r0 = 0; r0 < N; r0 += BH_ROWS) {
            for (int e = lane; e < NO * BH_ROWS; e += 64) mk[e] = 0ull;
            bh_wave_lds_fence();
#pragma unroll
            for (int q = 0; q < NO; ++q) {
                const int rel = ns[q] - r0;
                if (rel >= 0 && rel < BH_ROWS) atomicOr(&mk[rel * NO + q], 1ull << lane);
            }
            bh_wave_lds_fence();
            const int rend = (N - r0 < BH_ROWS ? N - r0 : BH_ROWS);
            const int j = lane % CPR;
            for (int rb = 0; rb < rend; rb += RG) {
                const int rel = rb + lane / CPR;
                const bool live = rel < rend;
                float acc[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = 0.f;
#pragma unroll
                for (int q = 0; q < NO; ++q) {
                    unsigned long long m = live ? mk[rel * NO + q] : 0ull;
                    while (m) {
                        const int o = __builtin_ctzll(m) + 64 * q;
                        m &= m - 1;
                        const float s = cfl[o];
                        const f32x4 w0 = *reinterpret_cast<const f32x4*>(Wl + o * LD + 8 * j);
                        const f32x4 w1 = *reinterpret_cast<const f32x4*>(Wl + o * LD + 8 * j + 4);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            acc[u] = fmaf(s, w0[u], acc[u]);
                            acc[4 + u] = fmaf(s, w1[u], acc[4 + u]);
                        }
                    }
                }
                if (live) bh_st8<PK>(gxb + (int64_t)(r0 + rel) * d.x_sn + (int64_t)(8 * j) * d.x_sc, d.x_sc, acc);
            }
            bh_wave_lds_fence();
        }
#ifdef FGNN_ENABLE_PROF
        if (first) BH_STAMP(3);
#endif

        // ---- dW[:, o] += c_o x[n*_o, :] ----
#pragma unroll
        for (int q = 0; q < NO; ++q)
#pragma unroll
            for (int i = 0; i < CPR; ++i) {
                float v[8];
                if constexpr (PRE) bh_unpack8<PK>(xraw[q][i], v);
                else bh_ld8<PK>(xb + (int64_t)ns[q] * d.x_sn + (int64_t)(8 * i) * d.x_sc, d.x_sc, v);
#pragma unroll
                for (int u = 0; u < 8; ++u) dW[q][8 * i + u] = fmaf(cf[q], v[u], dW[q][8 * i + u]);
            }
#ifdef FGNN_ENABLE_PROF
        if (first) BH_STAMP(4);
        first = false;
#endif
        bh_route_done<T, NO>(p, graw, nraw, eraw, g, ns, cf);
#pragma unroll
        for (int q = 0; q < NO; ++q) { graw[q] = graw2[q]; jraw[q] = jraw2[q]; }
        b = nb;
    }
    BH_STAMP(5);

    // ---- tail: every wave lays its sums down in a region of its own, then wave w adds the eight regions IN WAVE ORDER
    // (((w0 + w1) + w2) + ... + w7: the order the gradients have always been folded in — a parameter whose gradient is only
    // rounding noise, such as a bias in front of a BatchNorm, would otherwise take another Adam step) for its eighth of the
    // rows and writes them to the slab, lane <-> o: 256-byte rows.  The wide instances do it in two halves of the input
    // channels: eight regions of [CH][NOU] + [NOU] fit the LDS. ----
    constexpr int SL = NIN * NOU + NOU;
    constexpr int PASSES = NI * NO, CH = NIN / PASSES, RS = CH * NOU + NOU, RW = CH / BH_WAVES;
    float* fold = fgnn_lds_bh;
    float* slab = p.ws + (int64_t)blockIdx.x * SL + lane;
    __syncthreads();                                       // every wave is done with W^T, its masks and coefficients
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        float* mine = fold + wave * RS + lane;
#pragma unroll
        for (int q = 0; q < NO; ++q) {
#pragma unroll
            for (int c = 0; c < CH; ++c) mine[c * NOU + 64 * q] = dW[q][ps * CH + c];
            if (ps == 0) mine[CH * NOU + 64 * q] = gbv[q];
        }
        __syncthreads();
        const float* r = fold + lane;
#pragma unroll
        for (int q = 0; q < NO; ++q) {
#pragma unroll
            for (int cc = 0; cc < RW; ++cc) {
                const int c = wave * RW + cc;
                float t = r[c * NOU + 64 * q];
#pragma unroll
                for (int w = 1; w < BH_WAVES; ++w) t += r[w * RS + c * NOU + 64 * q];
                slab[(ps * CH + c) * NOU + 64 * q] = t;
            }
            if (ps == 0 && wave == 0) {
                float t = r[CH * NOU + 64 * q];
#pragma unroll
                for (int w = 1; w < BH_WAVES; ++w) t += r[w * RS + CH * NOU + 64 * q];
                slab[NIN * NOU + 64 * q] = t;
            }
        }
        if (ps + 1 < PASSES) __syncthreads();              // the regions are rewritten
        if (ps == 0) BH_STAMP(6);
    }
    BH_STAMP(7);
}

// ----------------------------------------------------------------------------------------
// fan-out: N == 1, k == 1, net == 1; gz channel-fastest [M][nou]
// ----------------------------------------------------------------------------------------
template <typename T, int NI, int NO>
__global__ __launch_bounds__(BH_THREADS) void mpconv_bwd_fanout_kernel(const BhParams p) {
    constexpr int NIN = 64 * NI, NOU = 64 * NO, CH = 4 * NO;
    const fgnn_mpconv_desc& d = p.d;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* Wl = fgnn_lds_bh;
    float* bl = Wl + NIN * NOU;
    bh_stage_w<NIN, NOU>(p.W, Wl, tid);
    __syncthreads();

    const T* X = reinterpret_cast<const T*>(p.x);
    const T* ET = reinterpret_cast<const T*>(p.et);
    const T* GZ = reinterpret_cast<const T*>(p.gz);
    T* GX = reinterpret_cast<T*>(p.gx);
    const int M = d.M;
    const int ch0 = (lane & 15) * CH, rc = lane >> 4;  // this lane's channels and row class of the gz sweep

    float dW[NI][NOU];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int o = 0; o < NOU; ++o) dW[i][o] = 0.f;
    float gbv[CH];
    int gbc[CH];
#pragma unroll
    for (int t = 0; t < CH; ++t) { gbv[t] = 0.f; gbc[t] = rc == 0 ? ch0 + t : -1; }

    const int nwaves = gridDim.x * BH_WAVES;
    for (int b = blockIdx.x * BH_WAVES + wave; b < d.B; b += nwaves) {
        float xv[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) xv[i] = fgnn_ld(X + (int64_t)b * d.x_sb + (int64_t)(lane + 64 * i) * d.x_sc);
        // dP[o] = sum_m et[m] gz[m, o]; dbias[o] += sum_m gz[m, o].  16 lanes x CH channels per row, 4 rows per sweep
        float dp[CH], bs[CH];
#pragma unroll
        for (int t = 0; t < CH; ++t) { dp[t] = 0.f; bs[t] = 0.f; }
        const T* gzb = GZ + (int64_t)b * d.y_sb + ch0;
        const T* etb = ET + (int64_t)b * d.et_sb;
        for (int r = rc; r < M; r += 4) {
            const float e = fgnn_ld(etb + (int64_t)r * d.et_sm);
#pragma unroll
            for (int h = 0; h < NO; ++h) {
                const f32x4 v = fgnn_ld4(gzb + (int64_t)r * d.y_sm + 4 * h);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    dp[4 * h + u] = fmaf(e, v[u], dp[4 * h + u]);
                    bs[4 * h + u] += v[u];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < CH; ++t) {
            dp[t] += __shfl_xor(dp[t], 16);
            dp[t] += __shfl_xor(dp[t], 32);
            bs[t] += __shfl_xor(bs[t], 16);
            bs[t] += __shfl_xor(bs[t], 32);
            gbv[t] += bs[t];
        }
        // dx = W dP, dW += x (x) dP   (lane <-> input channel; dP[o] lives in lane o / CH, register o % CH)
        float acc[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i] = 0.f;
#pragma unroll
        for (int o = 0; o < NOU; ++o) {
            const float s = fgnn_bcast(dp[o % CH], o / CH);
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                acc[i] = fmaf(s, Wl[o * NIN + lane + 64 * i], acc[i]);
                dW[i][o] = fmaf(s, xv[i], dW[i][o]);
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) fgnn_st(GX + (int64_t)b * d.x_sb + (int64_t)(lane + 64 * i) * d.x_sc, acc[i]);
    }
    bh_flush<NI, NO>(p, Wl, bl, dW, gbv, gbc, CH, tid, lane, wave);
}

// ----------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------
template <typename T>
static void* bh_pick(bool fanin, bool packed, int NI, int NO) {
#define BH_CASE(ni, no) if (NI == ni && NO == no) return !fanin ? (void*)mpconv_bwd_fanout_kernel<T, ni, no> : packed ? (void*)mpconv_bwd_fanin_kernel<T, ni, no, true> : (void*)mpconv_bwd_fanin_kernel<T, ni, no, false>;
    BH_CASE(1, 1) BH_CASE(1, 2) BH_CASE(2, 1)
#undef BH_CASE
    return nullptr;
}

static bool bh_aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// Constant-etype hyper-edge calls: one destination of degree N (fan-in, pl->mode 1) or one source (fan-out).
int fgnn_bwd_hyper_plan(const FgnnBwdCall& c, const FgnnSwitches&, FgnnPlan* pl) {
    const fgnn_mpconv_desc* d = c.d;
    if (c.getype) FGNN_REJECT("hyper-edge backward", 1);                 // edge-weight gradient: the resident kernel has it
    if (d->ext != FGNN_EXT_NONE || d->agg != FGNN_AGG_MAX || d->net != 1) FGNN_REJECT("hyper-edge backward", 2);
    if (d->nin % 64 || d->nou % 64 || d->nin > 128 || d->nou > 128 || d->nin * d->nou > 64 * 128) FGNN_REJECT("hyper-edge backward", 3);
    const bool fanin = d->M == 1 && d->k >= 1 && d->k <= 256 && d->N >= 1;
    const bool fanout = !fanin && d->N == 1 && d->k == 1;
    if (!fanin && !fanout) FGNN_REJECT("hyper-edge backward", 4);
    if (fanout && !(d->y_sc == 1 && d->y_sm % 4 == 0 && d->y_sb % 4 == 0 && d->y_sm >= d->nou)) FGNN_REJECT("hyper-edge backward", 5);
    const int64_t slab_len = (int64_t)d->nin * d->nou + d->nou;
    if (!c.workspace || c.workspace_bytes < 256 * slab_len * 4) FGNN_REJECT("hyper-edge backward", 6);
    const int NI = d->nin / 64, NO = d->nou / 64;
    // fan-in: x / gx channel-fastest in 16-byte aligned rows take the 16-byte accesses; every other layout runs the same kernel
    // with element accesses (nothing is turned down for its layout: the NCHW calls of the tests are this kernel's too)
    const bool packed = fanin && d->x_sc == 1 && d->x_sb % 8 == 0 && (d->N == 1 || d->x_sn % 8 == 0) &&
                        (!c.x || bh_aligned16(c.x)) && (!c.gx || bh_aligned16(c.gx));
    pl->fn = d->dtype == FGNN_F32 ? bh_pick<float>(fanin, packed, NI, NO) : bh_pick<bf16_t>(fanin, packed, NI, NO);
    if (!pl->fn) FGNN_REJECT("hyper-edge backward", 7);
    pl->mode = fanin;
    pl->lds = fanin ? bh_fanin_lds(NI, NO) : (int)(slab_len * 4);
    pl->grid = (d->B + BH_WAVES - 1) / BH_WAVES < 256 ? (d->B + BH_WAVES - 1) / BH_WAVES : 256;
    pl->block = BH_THREADS;
    return 1;
}

int fgnn_bwd_hyper_launch(const FgnnBwdCall& c, const FgnnPlan& pl) {
    const fgnn_mpconv_desc* d = c.d;
    const int64_t nw = (int64_t)d->nin * d->nou, slab_len = nw + d->nou;
    BhParams p;
    p.d = *d;
    p.x = c.x; p.idx = c.idx; p.et = c.et; p.W = c.W; p.gz = c.gz; p.argmax = c.argmax; p.gx = c.gx;
    p.ws = (float*)c.workspace; p.has_bias = c.gbias != nullptr;
    p.wvec = bh_aligned16(c.W);
    p.prof = pl.mode ? fgnn_prof_begin() : nullptr;
    fgnn_note_kernel("mpconv_bwd_%s_kernel<%s, %d, %d>", pl.mode ? "fanin" : "fanout", d->dtype ? "bf16_t" : "float", d->nin / 64, d->nou / 64);
    void* args[] = {(void*)&p};
    const int rc = fgnn_launch_fn("mpconv hyper-edge backward", pl.fn, dim3(pl.grid), dim3(pl.block), pl.lds, c.stream, args);
    fgnn_prof_print(p.prof, "fanin bwd", 0, 8, 8, 16);
    return rc ? rc : fgnn_launch_slab_reduce(p.ws, pl.grid, slab_len, nw, c.gW, c.gbias, c.stream);
}
