// Device helpers and limits shared by the sequence attention kernels: the causal core (seq_attn.hip) and its key-padding
// mode (seq_attn_keypad.hip).
#pragma once
#include "common.h"

namespace {

constexpr int SA_MAX_L = 128;
constexpr int SA_MAX_DH = 64;
constexpr int SA_ROWS = 64;       // query rows per wave

template <int DH>
__device__ __forceinline__ float sa_dot(const float (&a)[DH], const float *__restrict__ row) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(row + d);
        s += a[d] * t[0];
        s += a[d + 1] * t[1];
        s += a[d + 2] * t[2];
        s += a[d + 3] * t[3];
    }
    return s;
}

// rows [b L, b L + L) x columns [col, col + dh) of src -> tile [L][DH], zero beyond dh
template <int DH>
__device__ __forceinline__ void sa_stage(const float *__restrict__ src, int64_t ld, int64_t row0, int col, int L, int dh,
                                         float *tile) {
    for (int idx = threadIdx.x; idx < L * DH; idx += blockDim.x) {
        const int j = idx / DH, d = idx % DH;
        tile[idx] = d < dh ? src[(row0 + j) * ld + col + d] : 0.f;
    }
}

// the score of key j against the staged query: the same d order in both directions
__device__ __forceinline__ float sa_last_score(const float *qv, const float *__restrict__ krow, int dh, float sq, float kmj) {
    float s = 0.f;
    for (int d = 0; d < dh; ++d) s += qv[d] * krow[d];
    return s / sq + kmj;
}

static inline bool sa_fits(int L, int heads, int dh) { return L >= 1 && L <= SA_MAX_L && dh >= 1 && dh <= SA_MAX_DH && heads >= 1; }
static inline int sa_pad_dh(int dh) { return dh <= 4 ? 4 : dh <= 8 ? 8 : dh <= 16 ? 16 : dh <= 32 ? 32 : 64; }

}  // namespace

#define SA_DISPATCH(DHP, CALL) \
    switch (DHP) {             \
        case 4: CALL(4); break;   \
        case 8: CALL(8); break;   \
        case 16: CALL(16); break; \
        case 32: CALL(32); break; \
        default: CALL(64); break; \
    }
