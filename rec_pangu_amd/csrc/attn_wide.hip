// Self-attention over FEW tokens with ONE WIDE head, split form: the complement of attn_core.hip.  gfx950.
//   reference: layers/attention.py:63-101 (MultiHeadSelfAttention(input_dim) with H = 1, a = input_dim: no W_res), as
//   multi_task/aitm.py:33,64-66 uses it over T = 2 tokens of width 400, followed by torch.sum(., dim=1).
//
// The operands are attn_core.hip's: QKV = X . [Wq|Wk|Wv]^T from ONE rp_linear_fwd GEMM over the B*T token rows, row-major
// [B*T, ldq] with columns Q | K | V (each a wide), and the residual xres [B*T, ldr] = X itself.  H = 1, so the reference's
// raw-view head split is the identity.  Per sample
//     S[t,s] = q_t . k_s (/scale),  P = softmax_s(S - rowmax),  O_t = sum_s P[t,s] v_s,  Y_t = relu(O_t + xres_t)
//     out = Y [B, T, a]  (sum_tokens = 0)   or   sum_t Y_t [B, a]  (sum_tokens = 1: the [B, T, a] tensor is never written)
//
// attn_core.hip gives a lane one (head, query) ROW and keeps q[a], acc[a] in registers: a <= 16.  Here T is tiny and a is
// wide, so the lanes run ALONG a: one wave per sample, lane l owns columns l*V .. l*V+V-1 of every 64*V-wide pass (V = 4:
// dwordx4 loads when a, the row strides and the base addresses allow it, else V = 1).  The T*T dot products are per-lane
// partial sums over the passes + a butterfly reduction across the wave (fixed order: bit-identical from run to run); the
// T x T scores and probabilities live in registers (T is a template argument, every loop over tokens is unrolled).
// No LDS: nothing is shared between lanes but the T*T scalars.  Each operand is read once in the forward (Q, K in the
// score pass; V, xres in the output pass): 4*T*a*4 bytes in and a*4 (or T*a*4) bytes out per sample — HBM-bound.
// A row narrower than 64*V columns leaves lanes idle (a = 20: 5 of 64): the form exists for wide rows, narrow heads
// (a <= 16) belong to attn_core.hip.
//
// Backward (cotangent dY [B, T, a], or [B, a] shared by every token when sum_tokens): S, P and the ReLU mask are recomputed
// from QKV and xres — nothing was saved.  Pass 1: Q, K -> S, P.  Pass 2: V, xres, dY -> O_t, dO_t = dY_t [O_t + xres_t > 0],
// written as dxres_t; dV_s = sum_t P[t,s] dO_t; per-lane partials of dP[t,s] = dO_t . v_s, reduced across the wave.
// dS = P o (dP - sum_s P dP) / scale.  Pass 3: Q, K again (L2 hits) -> dq_t = sum_s dS[t,s] k_s, dk_s = sum_t dS[t,s] q_t.
// Every output element has exactly one writer; no atomics, nothing crosses samples.  The gradients of X and of the
// stacked weights are the usual dgrad / wgrad GEMMs on dQKV.
//
// Range (rp_attention_wide_fits): H == 1, 2 <= T <= 4 (T*T scores in registers), 1 <= a <= 65536.  int64 addressing.
#include "common.h"

#include <initializer_list>

#define AW_BLOCK 256  // 4 waves = 4 samples per workgroup
#define AW_MAXT 4
#define AW_MAXA 65536
#define AW_MAX_BLOCKS 4096

template <int V>
struct AwVec;
template <>
struct AwVec<1> {
    float v[1];
};
template <>
struct AwVec<4> {
    float v[4];
};

template <int V>
__device__ __forceinline__ AwVec<V> aw_load(const float *p) {
    AwVec<V> r;
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(p);
        r.v[0] = t[0], r.v[1] = t[1], r.v[2] = t[2], r.v[3] = t[3];
    } else {
        r.v[0] = p[0];
    }
    return r;
}
template <int V>
__device__ __forceinline__ void aw_store(float *p, const AwVec<V> &r) {
    if constexpr (V == 4) {
        f32x4 t;
        t[0] = r.v[0], t[1] = r.v[1], t[2] = r.v[2], t[3] = r.v[3];
        *reinterpret_cast<f32x4 *>(p) = t;
    } else {
        p[0] = r.v[0];
    }
}

// P = softmax over s of (q_t . k_s) * inv_scale for one sample; q0 = the sample's first QKV row
template <int T, int V>
__device__ __forceinline__ void aw_probs(const float *__restrict__ q0, int64_t ldq, int a, float inv_scale, int lane,
                                         float (&P)[T][T]) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int s = 0; s < T; ++s) P[t][s] = 0.f;
    for (int c = lane * V; c < a; c += 64 * V) {
        AwVec<V> q[T], k[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            q[t] = aw_load<V>(q0 + t * ldq + c);
            k[t] = aw_load<V>(q0 + t * ldq + a + c);
        }
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int s = 0; s < T; ++s)
#pragma unroll
                for (int j = 0; j < V; ++j) P[t][s] += q[t].v[j] * k[s].v[j];
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        float m = -INFINITY, l = 0.f;
#pragma unroll
        for (int s = 0; s < T; ++s) {
            P[t][s] = rp_lane_sum(P[t][s]) * inv_scale;
            m = fmaxf(m, P[t][s]);
        }
#pragma unroll
        for (int s = 0; s < T; ++s) {
            P[t][s] = expf(P[t][s] - m);
            l += P[t][s];
        }
        const float il = 1.f / l;
#pragma unroll
        for (int s = 0; s < T; ++s) P[t][s] *= il;
    }
}

// O_t + xres_t for the lane's V columns at c (the forward's value and the backward's ReLU mask: one piece of code)
template <int T, int V>
__device__ __forceinline__ void aw_pre(const float (&P)[T][T], const AwVec<V> (&v)[T], const AwVec<V> (&x)[T],
                                       AwVec<V> (&pre)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float o = 0.f;
#pragma unroll
            for (int s = 0; s < T; ++s) o += P[t][s] * v[s].v[j];
            pre[t].v[j] = o + x[t].v[j];
        }
}

template <int T, int V>
__global__ __launch_bounds__(AW_BLOCK) void attn_wide_fwd_kernel(const float *__restrict__ qkv, int64_t ldq,
                                                                  const float *__restrict__ xres, int64_t ldr, int a,
                                                                  float inv_scale, int sum_tokens,
                                                                  float *__restrict__ out, int64_t B) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (AW_BLOCK / 64);
    for (int64_t b = (int64_t)blockIdx.x * (AW_BLOCK / 64) + (threadIdx.x >> 6); b < B; b += nwaves) {
        const float *q0 = qkv + b * T * ldq, *x0 = xres + b * T * ldr;
        float P[T][T];
        aw_probs<T, V>(q0, ldq, a, inv_scale, lane, P);
        for (int c = lane * V; c < a; c += 64 * V) {
            AwVec<V> v[T], x[T], pre[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                v[t] = aw_load<V>(q0 + t * ldq + 2 * a + c);
                x[t] = aw_load<V>(x0 + t * ldr + c);
            }
            aw_pre<T, V>(P, v, x, pre);
            if (sum_tokens) {
                AwVec<V> y;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    float acc = 0.f;
#pragma unroll
                    for (int t = 0; t < T; ++t) acc += fmaxf(pre[t].v[j], 0.f);
                    y.v[j] = acc;
                }
                aw_store<V>(out + b * a + c, y);
            } else {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    AwVec<V> y;
#pragma unroll
                    for (int j = 0; j < V; ++j) y.v[j] = fmaxf(pre[t].v[j], 0.f);
                    aw_store<V>(out + (b * T + t) * a + c, y);
                }
            }
        }
    }
}

template <int T, int V>
__global__ __launch_bounds__(AW_BLOCK) void attn_wide_bwd_kernel(const float *__restrict__ qkv, int64_t ldq,
                                                                  const float *__restrict__ xres, int64_t ldr,
                                                                  const float *__restrict__ dout, int a, float inv_scale,
                                                                  int sum_tokens, float *__restrict__ dqkv, int64_t lddq,
                                                                  float *__restrict__ dxres, int64_t lddr, int64_t B) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (AW_BLOCK / 64);
    for (int64_t b = (int64_t)blockIdx.x * (AW_BLOCK / 64) + (threadIdx.x >> 6); b < B; b += nwaves) {
        const float *q0 = qkv + b * T * ldq, *x0 = xres + b * T * ldr;
        float *dq0 = dqkv + b * T * lddq, *dx0 = dxres + b * T * lddr;
        float P[T][T], dP[T][T];
        aw_probs<T, V>(q0, ldq, a, inv_scale, lane, P);
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int s = 0; s < T; ++s) dP[t][s] = 0.f;
        for (int c = lane * V; c < a; c += 64 * V) {
            AwVec<V> v[T], x[T], pre[T], go[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                v[t] = aw_load<V>(q0 + t * ldq + 2 * a + c);
                x[t] = aw_load<V>(x0 + t * ldr + c);
                go[t] = aw_load<V>(dout + (sum_tokens ? b * a : (b * T + t) * a) + c);
            }
            aw_pre<T, V>(P, v, x, pre);
#pragma unroll
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int j = 0; j < V; ++j) go[t].v[j] = pre[t].v[j] > 0.f ? go[t].v[j] : 0.f;  // dO_t
                aw_store<V>(dx0 + t * lddr + c, go[t]);
            }
#pragma unroll
            for (int s = 0; s < T; ++s) {
                AwVec<V> dv;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    float acc = 0.f;
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        acc += P[t][s] * go[t].v[j];
                        dP[t][s] += go[t].v[j] * v[s].v[j];
                    }
                    dv.v[j] = acc;
                }
                aw_store<V>(dq0 + s * lddq + 2 * a + c, dv);
            }
        }
        // dS (kept in dP)
#pragma unroll
        for (int t = 0; t < T; ++t) {
            float dot = 0.f;
#pragma unroll
            for (int s = 0; s < T; ++s) {
                dP[t][s] = rp_lane_sum(dP[t][s]);
                dot += P[t][s] * dP[t][s];
            }
#pragma unroll
            for (int s = 0; s < T; ++s) dP[t][s] = P[t][s] * (dP[t][s] - dot) * inv_scale;
        }
        for (int c = lane * V; c < a; c += 64 * V) {
            AwVec<V> q[T], k[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                q[t] = aw_load<V>(q0 + t * ldq + c);
                k[t] = aw_load<V>(q0 + t * ldq + a + c);
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                AwVec<V> dq, dk;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    float aq = 0.f, ak = 0.f;
#pragma unroll
                    for (int s = 0; s < T; ++s) {
                        aq += dP[t][s] * k[s].v[j];
                        ak += dP[s][t] * q[s].v[j];
                    }
                    dq.v[j] = aq;
                    dk.v[j] = ak;
                }
                aw_store<V>(dq0 + t * lddq + c, dq);
                aw_store<V>(dq0 + t * lddq + a + c, dk);
            }
        }
    }
}

extern "C" int rp_attention_wide_fits(int T, int H, int a) {
    return (H == 1 && T >= 2 && T <= AW_MAXT && a >= 1 && a <= AW_MAXA) ? 1 : 0;
}

static unsigned aw_grid(int64_t B) {
    const int64_t nb = rp_cdiv(B, AW_BLOCK / 64);
    return (unsigned)(nb < AW_MAX_BLOCKS ? nb : AW_MAX_BLOCKS);
}

// dwordx4 accesses need every row of every operand 16-byte aligned
static bool aw_vec4(int a, std::initializer_list<const void *> ptrs, std::initializer_list<int64_t> lds) {
    if (a % 4 != 0) return false;
    for (const void *p : ptrs)
        if (!rp_aligned16(p)) return false;
    for (int64_t ld : lds)
        if (ld % 4 != 0) return false;
    return true;
}

#define AW_DISPATCH(KERNEL, ...)                                                                                        \
    do {                                                                                                                \
        const dim3 grid(aw_grid(B)), block(AW_BLOCK);                                                                   \
        if (vec4) {                                                                                                     \
            if (T == 2) hipLaunchKernelGGL((KERNEL<2, 4>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);           \
            else if (T == 3) hipLaunchKernelGGL((KERNEL<3, 4>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);      \
            else hipLaunchKernelGGL((KERNEL<4, 4>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);                  \
        } else {                                                                                                        \
            if (T == 2) hipLaunchKernelGGL((KERNEL<2, 1>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);           \
            else if (T == 3) hipLaunchKernelGGL((KERNEL<3, 1>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);      \
            else hipLaunchKernelGGL((KERNEL<4, 1>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);                  \
        }                                                                                                               \
    } while (0)

extern "C" int rp_attention_wide_fwd(const float *qkv, int64_t ldq, const float *xres, int64_t ldr, int T, int H, int a,
                                     float scale, int sum_tokens, float *out, int64_t B, rp_stream_t stream) {
    RP_REQUIRE(qkv && xres && out, "attention_wide_fwd: null pointer");
    RP_REQUIRE(B >= 1, "attention_wide_fwd: empty batch");
    if (!rp_attention_wide_fits(T, H, a))
        return rp_fail(RP_ERR_UNSUPPORTED, "attention_wide: T=%d H=%d a=%d unsupported (H == 1, 2 <= T <= %d, 1 <= a <= %d)", T,
                       H, a, AW_MAXT, AW_MAXA);
    RP_REQUIRE(ldq >= 3 * (int64_t)a && ldr >= a, "attention_wide_fwd: a leading dimension is smaller than its row");
    const bool vec4 = aw_vec4(a, {qkv, xres, out}, {ldq, ldr});
    const float inv_scale = scale > 0.f ? 1.f / scale : 1.f;
    AW_DISPATCH(attn_wide_fwd_kernel, qkv, ldq, xres, ldr, a, inv_scale, sum_tokens ? 1 : 0, out, B);
    RP_LAUNCH_CHECK("attention_wide_fwd");
    return RP_OK;
}

extern "C" int rp_attention_wide_bwd(const float *qkv, int64_t ldq, const float *xres, int64_t ldr, const float *dout, int T,
                                     int H, int a, float scale, int sum_tokens, float *dqkv, int64_t lddq, float *dxres,
                                     int64_t lddr, int64_t B, rp_stream_t stream) {
    RP_REQUIRE(qkv && xres && dout && dqkv && dxres, "attention_wide_bwd: null pointer");
    RP_REQUIRE(B >= 1, "attention_wide_bwd: empty batch");
    if (!rp_attention_wide_fits(T, H, a))
        return rp_fail(RP_ERR_UNSUPPORTED, "attention_wide: T=%d H=%d a=%d unsupported (H == 1, 2 <= T <= %d, 1 <= a <= %d)", T,
                       H, a, AW_MAXT, AW_MAXA);
    RP_REQUIRE(ldq >= 3 * (int64_t)a && ldr >= a && lddq >= 3 * (int64_t)a && lddr >= a,
               "attention_wide_bwd: a leading dimension is smaller than its row");
    const bool vec4 = aw_vec4(a, {qkv, xres, dout, dqkv, dxres}, {ldq, ldr, lddq, lddr});
    const float inv_scale = scale > 0.f ? 1.f / scale : 1.f;
    AW_DISPATCH(attn_wide_bwd_kernel, qkv, ldq, xres, ldr, dout, a, inv_scale, sum_tokens ? 1 : 0, dqkv, lddq, dxres, lddr, B);
    RP_LAUNCH_CHECK("attention_wide_bwd");
    return RP_OK;
}
