// linear_wgrad_f32.hip — f32 weight / bias gradient of the node-wise (1x1) maps for the synthetic-PGM models (f32 storage,
// rows = B * nodes ~ 6e4, channel counts 64..512: /root/reference/lib/model/mpnn/factor_mpnn.py:40-70, mp_nn_residual.py:25-35):
//
//     gW[o][c] += sum_r gy[r][o] * x[r][c]        gb[o] += sum_r gy[r][o]
//
// The general kernel of linear_wgrad.hip stages 32-row tiles for 4 waves that own up to 16 output tiles each and runs the wide
// maps of these models at 0.4-0.8 TB/s (256 x 256: 315 us where the f32 matrix cores need 57 us and the bytes 25 us).  Here
// the OUTPUT is blocked (up to 128 x 128 per workgroup, 8 waves of 16 x 16 tiles in registers), the rows are split over the x
// dimension of the grid and the next 32-row tile travels in registers.  Per-chunk partial blocks go to slabs that a second
// kernel folds in a fixed order (no atomics: bit-reproducible).
#include "linear_wgrad.h"
#include "fgnn_device.h"

#define WF_THREADS 512
#define WF_TR 32             // rows per LDS tile (8 k-steps)
#define WF_BLK 128           // output block: 128 output channels x 128 input channels

struct WfParams {
    const float* x;          // [R][Cin]
    const float* gy;         // [R][Cout]
    float* ws;               // [nrc][Cout * Cin + Cout]
    int R, Cin, Cout;
    int rows_per_chunk, nblk_c;
    int want_bias;
};

// ---------------------------------------------------------------------------------------------------------------------------
// Piece form (round 6): the blocked product on the bf16 matrix cores.  Its f32 matrix-core predecessor (removed: git history,
// DESIGN §4.12b) was bound by the f32 matrix pipe (64 v_mfma_f32_16x16x4_f32 = 2 048 cycles per wave and 32-row tile; a 64 x 64
// map padded its 128 x 128 block to a quarter full): 29 us per map at the synthetic-PGM models' 61 440 rows, 38 maps per training step = 8 % of BASELINE config 5's step.  Here a
// tile's operands are cut into three bf16 pieces when they are committed to LDS (h + m + l: 2^-24, the arithmetic of
// mpconv_fwd_extp_kernel) and both operands — gy^T and x, contracted over the tile's 32 ROWS — come out of the row-major piece
// images through ds_read_b64_tr_b16 (256-byte rows, 32-byte segments swizzled by (r & 3) | (r >> 3 & 1) << 2: conflict-free
// transpose passes): one k-step of v_mfma_f32_16x16x32_bf16 per tile, 8 fragment products x 6 piece products = 768 cycles.
// The bias gradient is summed from the f32 registers at commit time.
// ---------------------------------------------------------------------------------------------------------------------------
#define WQ_NP 3
#define WQ_ROW 256                      // bytes per image row: 128 bf16
#define WQ_PIECE (WF_TR * WQ_ROW)       // one piece image of a 32-row tile

__device__ __forceinline__ int wq_sw(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }

// BO x BC = the output block (64 or 128 each: a 64-channel side takes a 64-wide block instead of padding a 128-wide one);
// waves = 4 (o) x 2 (c): BO / 64 o tiles and BC / 32 c tiles per wave
template <int BO, int BC>
__global__ __launch_bounds__(WF_THREADS, 2) void linear_wgrad_f32q_kernel(const WfParams p) {
    constexpr int GROW = 2 * BO, XROW = 2 * BC;                      // image row bytes
    constexpr int GPIECE = WF_TR * GROW, XPIECE = WF_TR * XROW;
    constexpr int NO = BO / 64, NC = BC / 32;                         // tiles per wave
    constexpr int GCH = BO / 4, XCH = BC / 4;                         // 16-byte chunks (4 floats) per tile row
    constexpr int GPT = WF_TR * GCH / WF_THREADS, XPT = WF_TR * XCH / WF_THREADS;     // chunks per thread and tile (1 or 2)
    constexpr int RG = WF_THREADS / GCH;                              // row groups of the gy staging (bias partials)
    __shared__ __attribute__((aligned(16))) unsigned char gq[WQ_NP * GPIECE];      // gy pieces [piece][32 rows][BO]
    __shared__ __attribute__((aligned(16))) unsigned char xq[WQ_NP * XPIECE];      // x pieces  [piece][32 rows][BC]
    __shared__ float bpart[RG * BO];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int bo = blockIdx.y / p.nblk_c, bc = blockIdx.y - bo * p.nblk_c;
    const int o0 = bo * BO, c0 = bc * BC;
    const int Cin = p.Cin, Cout = p.Cout;
    const int wo = wave & 3, wc = wave >> 2;              // o tiles NO wo ..; c tiles NC wc ..
    const unsigned gq0 = (unsigned)(uintptr_t)gq, xq0 = (unsigned)(uintptr_t)xq;
    // 32-byte segment swizzles (conflict-free transpose passes over rows {r..r+3, r+8..r+11}): 256-byte rows / 128-byte rows
    auto swz = [](int r, int rowbytes) { return rowbytes == 256 ? ((r & 3) | (((r >> 3) & 1) << 2)) : (((r >> 1) & 1) | (((r >> 3) & 1) << 1)); };

    const int r_begin = blockIdx.x * p.rows_per_chunk;
    const int r_end = min(p.R, r_begin + p.rows_per_chunk);

    uint4 pg[GPT], px[XPT];
    auto prefetch = [&](int r0) {
#pragma unroll
        for (int i = 0; i < GPT; ++i) {
            const int q = tid + i * WF_THREADS, row = q / GCH, col = (q % GCH) * 4;
            const int r = r0 + row;
            pg[i] = (r < r_end && o0 + col < Cout) ? *reinterpret_cast<const uint4*>(p.gy + (int64_t)r * Cout + o0 + col) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int q = tid + i * WF_THREADS, row = q / XCH, col = (q % XCH) * 4;
            const int r = r0 + row;
            px[i] = (r < r_end && c0 + col < Cin) ? *reinterpret_cast<const uint4*>(p.x + (int64_t)r * Cin + c0 + col) : make_uint4(0, 0, 0, 0);
        }
    };
    float bs[4] = {0.f, 0.f, 0.f, 0.f};                   // bias gradient: this thread's four gy columns, over its rows
    auto put = [&](unsigned char* img, int piece, int rowbytes, int row, int col, const uint4& v) {
        float a = __uint_as_float(v.x), b = __uint_as_float(v.y), c = __uint_as_float(v.z), d = __uint_as_float(v.w);
        unsigned char* dst = img + row * rowbytes + (((col >> 4) ^ swz(row, rowbytes)) << 5) + ((col & 15) << 1);
#pragma unroll
        for (int t = 0; t < WQ_NP; ++t) {
            const unsigned w0 = fgnn_pack2(a, b), w1 = fgnn_pack2(c, d);
            *reinterpret_cast<uint2*>(dst + t * piece) = make_uint2(w0, w1);
            if (t + 1 < WQ_NP) {
                a -= __uint_as_float(w0 << 16); b -= __uint_as_float(w0 & 0xffff0000u);
                c -= __uint_as_float(w1 << 16); d -= __uint_as_float(w1 & 0xffff0000u);
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < GPT; ++i) {
            const int q = tid + i * WF_THREADS, row = q / GCH, col = (q % GCH) * 4;
            bs[0] += __uint_as_float(pg[i].x); bs[1] += __uint_as_float(pg[i].y); bs[2] += __uint_as_float(pg[i].z); bs[3] += __uint_as_float(pg[i].w);
            put(gq, GPIECE, GROW, row, col, pg[i]);
        }
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int q = tid + i * WF_THREADS, row = q / XCH, col = (q % XCH) * 4;
            put(xq, XPIECE, XROW, row, col, px[i]);
        }
    };

    f32x4 acc[NO][NC];
#pragma unroll
    for (int a = 0; a < NO; ++a)
#pragma unroll
        for (int b = 0; b < NC; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // transpose-read addresses: lane (li, lk) names rows 8 lk + (li >> 2) (+ 4), four columns from 4 (li & 3) of a 16-column segment
    const int r0t = 8 * lk + (li >> 2), r1t = r0t + 4;
    const unsigned g0 = r0t * GROW + ((li & 3) << 3), g1 = r1t * GROW + ((li & 3) << 3);
    const unsigned x0 = r0t * XROW + ((li & 3) << 3), x1 = r1t * XROW + ((li & 3) << 3);
    const int sg0 = swz(r0t, GROW), sg1 = swz(r1t, GROW), sx0 = swz(r0t, XROW), sx1 = swz(r1t, XROW);
    constexpr int TA[6] = {2, 0, 1, 1, 0, 0}, TB[6] = {0, 2, 1, 0, 1, 0};     // smallest piece products first

    if (r_begin < r_end) prefetch(r_begin);
    for (int r0 = r_begin; r0 < r_end; r0 += WF_TR) {
        __syncthreads();                                  // the previous tile's operands have been read
        commit();
        if (r0 + WF_TR < r_end) prefetch(r0 + WF_TR);
        __syncthreads();
        bf16x8 ga[NO][WQ_NP], xb[NC][WQ_NP];
#pragma unroll
        for (int a = 0; a < NO; ++a)
#pragma unroll
            for (int t = 0; t < WQ_NP; ++t) {
                const int g = NO * wo + a;
                const uint2 lo = fgnn_tr16(gq0 + t * GPIECE + g0 + ((g ^ sg0) << 5)), hi = fgnn_tr16(gq0 + t * GPIECE + g1 + ((g ^ sg1) << 5));
                ga[a][t] = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
            }
#pragma unroll
        for (int b = 0; b < NC; ++b)
#pragma unroll
            for (int t = 0; t < WQ_NP; ++t) {
                const int g = NC * wc + b;
                const uint2 lo = fgnn_tr16(xq0 + t * XPIECE + x0 + ((g ^ sx0) << 5)), hi = fgnn_tr16(xq0 + t * XPIECE + x1 + ((g ^ sx1) << 5));
                xb[b][t] = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
            }
#pragma unroll
        for (int pr6 = 0; pr6 < 6; ++pr6)
#pragma unroll
            for (int a = 0; a < NO; ++a)
#pragma unroll
                for (int b = 0; b < NC; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga[a][TA[pr6]], xb[b][TB[pr6]], acc[a][b], 0, 0, 0);
    }

    // D[i = o (4 lk + r)][j = c (li)] of tile (ot, ct) -> this chunk's slab, in gW's own layout
    float* slab = p.ws + (int64_t)blockIdx.x * ((int64_t)Cout * Cin + Cout);
#pragma unroll
    for (int a = 0; a < NO; ++a)
#pragma unroll
        for (int b = 0; b < NC; ++b) {
            const int c = c0 + (NC * wc + b) * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = o0 + (NO * wo + a) * 16 + 4 * lk + r;
                if (o < Cout && c < Cin) slab[(int64_t)o * Cin + c] = acc[a][b][r];
            }
        }
    if (p.want_bias && bc == 0) {                         // the row groups' column sums, folded in a fixed order
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) bpart[(tid / GCH) * BO + 4 * (tid % GCH) + e] = bs[e];
        __syncthreads();
        if (tid < BO && o0 + tid < Cout) {
            float sum = 0.f;
#pragma unroll
            for (int g = 0; g < RG; ++g) sum += bpart[g * BO + tid];
            slab[(int64_t)Cout * Cin + o0 + tid] = sum;
        }
    }
}

// ---- host: the f32 family of the dispatch (linear_wgrad.h) ----

// >= 2048 rows, channel counts multiples of 4 in 16..1024; maps narrower than 64 x 64 stay with the general kernel (one block
// would be mostly padding)
int fgnn_wgrad_f32_plan(const FgnnWgradCall& c, FgnnWgradPlan* pl) {
    const int64_t R = c.R;
    const int Cin = c.Cin, Cout = c.cout[0];
    if (R < 2048 || R > 0x7fffffff || Cin % 4 || Cout % 4 || Cin < 16 || Cout < 16 || Cin > 1024 || Cout > 1024 || (int64_t)Cin * Cout < 4096)
        FGNN_REJECT("wgrad f32", 1);
    if (c.x && (((uintptr_t)c.x & 15) || ((uintptr_t)c.gy[0] & 15))) FGNN_REJECT("wgrad f32", 2);
    const int nblk_o = (Cout + WF_BLK - 1) / WF_BLK;      // (a side of <= 64 channels is ONE block in both block sizes: the plan does not
    pl->aux = (Cin + WF_BLK - 1) / WF_BLK;                //  depend on the form that runs)
    int target = 256 / (nblk_o * pl->aux);                // one workgroup per CU: enough for the chip, and the slab traffic stays down
    if (target < 1) target = 1;
    int64_t rows = (R + target - 1) / target;
    if (rows < 2 * WF_TR) rows = 2 * WF_TR;
    rows = (rows + WF_TR - 1) / WF_TR * WF_TR;
    pl->rows = (int)rows;
    pl->gx = (int)((R + rows - 1) / rows);
    pl->gy = nblk_o * pl->aux;
    pl->ws_bytes = (int64_t)pl->gx * ((int64_t)Cout * Cin + Cout) * 4;
    return 1;
}

// The piece-form kernel of a map: a side of <= 64 channels takes a 64-wide block.  Chosen here for the launch and for the name.
enum { WQ_64x64, WQ_64x128, WQ_128x64, WQ_128x128 };
static int wq_form(int Cin, int Cout) {
    if (Cout <= 64 && Cin <= 64) return WQ_64x64;
    if (Cout <= 64) return WQ_64x128;
    return Cin <= 64 ? WQ_128x64 : WQ_128x128;
}

const char* fgnn_wgrad_f32_name(const FgnnWgradCall& c, const FgnnWgradPlan&) {
    static const char* const names[] = {"linear_wgrad_f32q_kernel<64, 64>", "linear_wgrad_f32q_kernel<64, 128>",
                                        "linear_wgrad_f32q_kernel<128, 64>", "linear_wgrad_f32q_kernel<128, 128>"};
    return names[wq_form(c.Cin, c.cout[0])];
}

int fgnn_wgrad_f32_launch(const FgnnWgradCall& c, const FgnnWgradPlan& pl) {
    const int Cin = c.Cin, Cout = c.cout[0];
    const int64_t nw = (int64_t)Cout * Cin, slab_len = nw + Cout;
    WfParams p;
    p.x = (const float*)c.x; p.gy = (const float*)c.gy[0]; p.ws = (float*)c.workspace; p.R = (int)c.R; p.Cin = Cin; p.Cout = Cout;
    p.rows_per_chunk = pl.rows; p.nblk_c = pl.aux; p.want_bias = c.gb[0] != nullptr;
    const dim3 grid(pl.gx, pl.gy), block(WF_THREADS);
    void (*kernel)(WfParams);
    switch (wq_form(Cin, Cout)) {
    case WQ_64x64: kernel = linear_wgrad_f32q_kernel<64, 64>; break;
    case WQ_64x128: kernel = linear_wgrad_f32q_kernel<64, 128>; break;
    case WQ_128x64: kernel = linear_wgrad_f32q_kernel<128, 64>; break;
    default: kernel = linear_wgrad_f32q_kernel<128, 128>; break;
    }
    const int rc = fgnn_launch("linear_wgrad f32", kernel, grid, block, 0, c.stream, p);
    return rc ? rc : fgnn_launch_slab_reduce(p.ws, pl.gx, slab_len, nw, c.gW[0], c.gb[0], c.stream);
}
