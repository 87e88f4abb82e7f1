// The skeleton the two score-tile loss files share (softmax_ce.hip, contrast.hip; included by nothing else): a loss over a
// [rows, cols] score matrix that never exists, formed 32 x 32 tiles at a time in the matrix core's accumulators by a
// workgroup of 4 waves, the columns cut into splits.  Here, once: the tile and split constants, the fragment loads, the
// wave add, a split's tile range, the two finishing kernels both files launch unchanged (the mean and the split-order slab reduce) and the host's
// split plan, product count, fast-load test and (DT, NPROD) dispatch.  Each file keeps what really differs: its per-element
// transform, its workspace layout, its finish kernel, its merge function and its entry points.
//
// Two things are decided here for both files.  The recomputed tile carries the forward's bits (softmax_ce.hip's header has
// the -lse seeding finding), so a backward forms its scores with the forward's piece pairs in the forward's order.  And the
// register budget: D <= ST_MAX_D, the contraction zero-padded to a multiple of 32; above, the pieces of the resident operand
// and the D / 32 output accumulators no longer fit beside the score tile without spilling.
//
// Everything below has internal linkage: each including file compiles its own copy of the two kernels.
#pragma once
#include "common.h"
#include "bfsplit.h"

#define ST_TILE 32         // rows and columns of a score tile
#define ST_WAVES 4
#define ST_BLOCK 256
#define ST_MAX_D 128
#define ST_MAX_SPLITS 64
#define ST_MIN_TILES 4     // tiles per split at least: one per wave
#define ST_FILL 1024       // workgroups the split of the columns aims at

namespace {

// 8 consecutive floats of one row from column c on, zero beyond D / for a row outside the matrix
__device__ __forceinline__ f32x8 st_load8(const float *__restrict__ base, int64_t ld, int64_t row, bool valid, int c, int D,
                                          bool fast) {
    f32x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (valid && c < D) {
        const float *p = base + row * ld + c;
        if (fast) {  // D % 16 == 0: c + 8 <= D
            const f32x4 a = *reinterpret_cast<const f32x4 *>(p), b = *reinterpret_cast<const f32x4 *>(p + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = a[j];
                v[4 + j] = b[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c + j < D) v[j] = p[j];
        }
    }
    return v;
}

// the operand that meets an accumulator tile used as a fragment: element j of k-step s is the tile row
// rp_mfma32_row(8 s + j, h)
// (cdna4: registers 8s .. 8s+7 of the accumulator are rows 16 s + 8 (j >> 2) + 4 h + (j & 3)); column c of `base`
__device__ __forceinline__ f32x8 st_load_rows(const float *__restrict__ base, int64_t ld, int64_t row0, int64_t nrows, int s,
                                              int h, int c, int D) {
    f32x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t row = row0 + rp_mfma32_row(8 * s + j, h);
        v[j] = (row < nrows && c < D) ? base[row * ld + c] : 0.f;
    }
    return v;
}

// the four waves' accumulators hold the same (register, lane) layout: waves 1..3 park theirs in LDS, wave 0 adds them in
// wave order
template <int DT>
__device__ __forceinline__ void st_add_waves(f32x16 (&acc)[DT], float *red, int w, int lane) {
    if (w > 0) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) red[(((w - 1) * DT + dt) * 16 + i) * 64 + lane] = acc[dt][i];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int q = 0; q < ST_WAVES - 1; ++q)
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[dt][i] += red[((q * DT + dt) * 16 + i) * 64 + lane];
    }
}

// the column tiles [t0, t1) of split blockIdx.y, tps tiles per split (the last split may hold fewer)
struct StTiles {
    int64_t t0, t1;
};
__device__ __forceinline__ StTiles st_split_tiles(int64_t cols, int64_t tps) {
    const int64_t tiles = (cols + ST_TILE - 1) / ST_TILE;
    const int64_t t0 = (int64_t)blockIdx.y * tps;
    return {t0, (t0 + tps < tiles) ? t0 + tps : tiles};
}

// loss = coef * the sum of the finish kernel's per-workgroup sums, added in a fixed order (one workgroup)
__global__ __launch_bounds__(ST_BLOCK) void st_mean_kernel(const float *__restrict__ partial, int64_t nb, float coef,
                                                           float *__restrict__ loss) {
    __shared__ float sh[ST_WAVES];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < nb; i += ST_BLOCK) s += partial[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = __fmul_rn((sh[0] + sh[1]) + (sh[2] + sh[3]), coef);
}

// out[i, d] = g coef (sum over the splits' [n, D] slabs, in split order, + extra[i, d]); extra NULL or one more unscaled
// [n, D] addend (contrast.hip's symmetric form)
__global__ __launch_bounds__(ST_BLOCK) void st_slab_reduce_kernel(const float *__restrict__ slabs, int nsplit, int64_t n, int D,
                                                                  const float *__restrict__ extra,
                                                                  const float *__restrict__ gloss, float coef,
                                                                  float *__restrict__ out, int64_t ldo) {
    const float scale = gloss[0] * coef;
    const int64_t total = n * D;
    for (int64_t e = (int64_t)blockIdx.x * ST_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * ST_BLOCK) {
        float s = slabs[e];
        for (int sp = 1; sp < nsplit; ++sp) s += slabs[(int64_t)sp * total + e];
        if (extra) s += extra[e];
        const int64_t i = e / D;
        out[i * ldo + (e - i * D)] = s * scale;
    }
}

// ---- host

struct StPlan {
    int64_t row_tiles, tiles, tps;  // tiles of rows, tiles of columns, column tiles per split
    int nsplit;
};

// the split of the columns: as many splits as bring the grid to ST_FILL workgroups, at most ST_MAX_SPLITS, each of at
// least ST_MIN_TILES tiles; the last split may hold fewer
StPlan st_plan(int64_t rows, int64_t cols) {
    StPlan g;
    g.row_tiles = rp_cdiv(rows, ST_TILE);
    g.tiles = rp_cdiv(cols, ST_TILE);
    int64_t want = rp_cdiv(ST_FILL, g.row_tiles);
    if (want > ST_MAX_SPLITS) want = ST_MAX_SPLITS;
    if (want < 1) want = 1;
    g.tps = rp_cdiv(g.tiles, want);
    if (g.tps < ST_MIN_TILES) g.tps = ST_MIN_TILES;
    g.nsplit = (int)rp_cdiv(g.tiles, g.tps);
    return g;
}

// the product count of the GEMM a launch stands for (the scores included, as rp_linear_fwd counts its output);
// RP_MATMUL_FP32 (a count of 0) runs 6: there is no f32-MFMA form
int st_products(int64_t rows, int64_t cols, int D) {
    const int np = rp_matmul_products(2.0 * rows * cols * D, 4.0 * ((double)rows * D + (double)cols * D + (double)rows * cols));
    return np == 0 ? 6 : np;
}

// st_load8 may read a row as two dwordx4
bool st_fast(const float *p, int64_t ld, int D) { return D % 16 == 0 && ld % 4 == 0 && rp_aligned16(p); }

}  // namespace

// CALL(DT, NPROD) for DT = ceil(D / 32) in 1..4 and NPROD in {1, 3, 6}
#define ST_DISPATCH(DT_, NPROD_, CALL)                           \
    do {                                                         \
        switch ((DT_) * 8 + (NPROD_)) {                          \
            case 1 * 8 + 1: { CALL(1, 1); } break;               \
            case 1 * 8 + 3: { CALL(1, 3); } break;               \
            case 1 * 8 + 6: { CALL(1, 6); } break;               \
            case 2 * 8 + 1: { CALL(2, 1); } break;               \
            case 2 * 8 + 3: { CALL(2, 3); } break;               \
            case 2 * 8 + 6: { CALL(2, 6); } break;               \
            case 3 * 8 + 1: { CALL(3, 1); } break;               \
            case 3 * 8 + 3: { CALL(3, 3); } break;               \
            case 3 * 8 + 6: { CALL(3, 6); } break;               \
            case 4 * 8 + 1: { CALL(4, 1); } break;               \
            case 4 * 8 + 3: { CALL(4, 3); } break;               \
            default: { CALL(4, 6); } break;                      \
        }                                                        \
    } while (0)
