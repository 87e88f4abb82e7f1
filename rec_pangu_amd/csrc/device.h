// Device helpers every kernel file shares (included from common.h): lane reductions, the 256-thread block sum, the Philox
// generator behind every dropout mask, the MFMA 32x32 accumulator row map, the fp32 row-by-row matrix-core product, sigmoid
// and a round-up.  A kernel file uses
// these and defines no copy of its own: a correction then reaches every kernel at once.
#pragma once

#define RP_WAVE 64  // wave64: hard-coded, gfx950 only

// ---- lane reductions over groups of G consecutive lanes (G a power of two, <= 64); every lane of a group ends with the
// group's result.  The DESCENDING butterfly (offsets G/2 .. 1) and the ASCENDING one (offsets 1 .. G/2) add in different
// orders and give different bits: they are two names on purpose, and a call site keeps the one it has.
template <int G = RP_WAVE, typename T>
__device__ __forceinline__ T rp_lane_sum(T v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}
template <int G = RP_WAVE>
__device__ __forceinline__ float rp_lane_max(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, G));
    return v;
}
template <int G = RP_WAVE, typename T>
__device__ __forceinline__ T rp_lane_sum_up(T v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v += __shfl_xor(v, m, G);
    return v;
}

// ---- sum over a 256-thread workgroup through sh[4]: wave butterflies, then (sh[0] + sh[1]) + (sh[2] + sh[3]).  The result
// is valid on THREAD 0 only (0 elsewhere); the trailing barrier frees sh for the next call.
__device__ __forceinline__ float rp_block_sum_256(float v, float *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // rp_lane_sum written out: as a nested call it reorders loss.hip's code
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x == 0) r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return r;
}

// ---- Philox4x32-10: THE random stream of the library (dropout.hip, seq_attn.hip).  Stateless: counter (c0..c3), key
// (k0, k1) -> four uniform 32-bit draws.  Each caller lays out its own counter (group, call offset) and key (seed).
__device__ __forceinline__ void rp_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                 uint32_t (&out)[4]) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0;
        c1 = n1;
        c2 = n2;
        c3 = n3;
        k0 += W0;
        k1 += W1;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}
// keep <=> r >= thresh with r uniform on [0, 2^32): P(drop) = thresh / 2^32 = p
static inline uint32_t rp_keep_thresh(float p) {
    double t = (double)p * 4294967296.0;
    if (t > 4294967295.0) t = 4294967295.0;
    return (uint32_t)t;
}

// row of element i (0..15) of a lane's v_mfma_f32_32x32 accumulator; h = lane / 32, the column is lane % 32
__device__ __forceinline__ int rp_mfma32_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// exact-fp32 matrix core, both operands read by rows (attn_pool.hip, session_graph.hip):
// acc += A[row, :] . W[col, :] over Kp columns (a multiple of 8); arow NULL or columns >= kvalid (a multiple of 4) read as zero
__device__ __forceinline__ f32x16 rp_mma_f32_rows(f32x16 acc, const float *arow, int Kp, int kvalid, const float *__restrict__ wrow,
                                                  int h) {
    for (int kq = 0; kq < Kp / 8; ++kq) {
        const int k = kq * 8 + 4 * h;
        f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
        if (arow != nullptr && k < kvalid) a4 = *reinterpret_cast<const f32x4 *>(arow + k);
        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(wrow + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b4[e], acc, 0, 0, 0);
    }
    return acc;
}

__device__ __forceinline__ float rp_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// host: n rounded up to a multiple of m (n >= 0, m > 0)
static inline int64_t rp_round_up(int64_t n, int64_t m) { return (n + m - 1) / m * m; }
