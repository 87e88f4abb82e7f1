// Row-wise LayerNorm over fp32 [M, N] (nn.LayerNorm over the last dimension, biased variance), with an optional
// elementwise multiplier behind it, gfx950.
//
// rp_layernorm_*  reference: layers/interaction.py:269-283 (MaskBlock: LN_in(net) * mask, LN_out(hidden)) and
//                 ranking/masknet.py:70-79 (the mean over parallel blocks: out_scale + accumulate).
//
// A wave64 owns a row.  Up to N = 2048 the row lives in registers (lane l holds the column quads l, l + 64, ...: NV quads
// per lane, one dwordx4 load each when the pointer and the leading dimension allow, per-element loads otherwise and in the
// last, partial quad); above that the same code walks the row from memory once per pass.  The statistics are two-pass:
// the mean first, then the sum of squared distances to it — never E[x^2] - mean^2.  All reductions have a fixed order
// (xor butterfly inside the wave; the column sums of the backward through per-wave partial rows in the workspace and a
// second launch): no floating-point atomics, bit-identical from run to run.
#include "common.h"

#define LN_VX 1    // x
#define LN_VMUL 2  // mul
#define LN_VY 4    // y / dx
#define LN_VP 8    // gamma and beta
#define LN_VDY 16  // dy
#define LN_VDM 32  // dmul

#define LN_FWD_BLOCKS 2048  // grid cap of the forward (4 rows per block, grid-stride over the rest)
#define LN_BWD_BLOCKS 512   // grid cap of the backward: 4 * 512 partial rows of (dgamma, dbeta) in the workspace

__device__ __forceinline__ f32x4 ln_load4(const float *__restrict__ p, int c, int N, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec && c + 4 <= N) {
        v = *reinterpret_cast<const f32x4 *>(p + c);
    } else {
        if (c < N) v.x = p[c];
        if (c + 1 < N) v.y = p[c + 1];
        if (c + 2 < N) v.z = p[c + 2];
        if (c + 3 < N) v.w = p[c + 3];
    }
    return v;
}

__device__ __forceinline__ void ln_store4(float *__restrict__ p, int c, int N, bool vec, f32x4 v) {
    if (vec && c + 4 <= N) {
        *reinterpret_cast<f32x4 *>(p + c) = v;
    } else {
        if (c < N) p[c] = v.x;
        if (c + 1 < N) p[c + 1] = v.y;
        if (c + 2 < N) p[c + 2] = v.z;
        if (c + 3 < N) p[c + 3] = v.w;
    }
}

// 1 for the columns of the quad at c that exist
__device__ __forceinline__ f32x4 ln_valid4(int c, int N) {
    f32x4 v = {c < N ? 1.f : 0.f, c + 1 < N ? 1.f : 0.f, c + 2 < N ? 1.f : 0.f, c + 3 < N ? 1.f : 0.f};
    return v;
}

__device__ __forceinline__ float ln_hsum(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }

// y = out_scale * ((gamma * (x - mu) * r + beta) [* mul])  [+ y];  NV = quads per lane held in registers, 0 = re-read
template <int NV>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const float *__restrict__ x, int64_t ldx,
                                                            const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, float eps,
                                                            const float *__restrict__ mul, int64_t ldmul, float *y,
                                                            int64_t ldy, int N_pad, float out_scale, int accumulate,
                                                            float *stats, int stats_given, int64_t M, int N, int vf) {
    const int lane = threadIdx.x & (RP_WAVE - 1);
    const int64_t w0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), W = (int64_t)gridDim.x * 4;
    const int nq = NV > 0 ? NV : (N + 255) / 256;
    const float invN = 1.f / (float)N;
    const bool vx = vf & LN_VX, vm = vf & LN_VMUL, vy = vf & LN_VY, vp = vf & LN_VP;
    for (int64_t m = w0; m < M; m += W) {
        const float *xr = x + m * ldx;
        f32x4 xv[NV > 0 ? NV : 1];
        if (NV > 0) {
#pragma unroll
            for (int j = 0; j < nq; ++j) xv[j] = ln_load4(xr, (j * RP_WAVE + lane) * 4, N, vx);
        }
        float mu, r;
        if (stats_given) {
            mu = stats[2 * m];
            r = stats[2 * m + 1];
        } else {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < nq; ++j) {
                const f32x4 v = NV > 0 ? xv[j] : ln_load4(xr, (j * RP_WAVE + lane) * 4, N, vx);
                s += ln_hsum(v);  // (columns that do not exist were loaded as 0)
            }
            mu = rp_lane_sum(s) * invN;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < nq; ++j) {
                const int c = (j * RP_WAVE + lane) * 4;
                const f32x4 v = NV > 0 ? xv[j] : ln_load4(xr, c, N, vx);
                const f32x4 d = (v - mu) * ln_valid4(c, N);
                q += ln_hsum(d * d);
            }
            r = 1.f / sqrtf(rp_lane_sum(q) * invN + eps);
            if (stats != nullptr && lane == 0) {
                stats[2 * m] = mu;
                stats[2 * m + 1] = r;
            }
        }
        float *yr = y + m * ldy;
        const float *mr = mul != nullptr ? mul + m * ldmul : nullptr;
#pragma unroll
        for (int j = 0; j < nq; ++j) {
            const int c = (j * RP_WAVE + lane) * 4;
            if (c < N) {
                const f32x4 v = NV > 0 ? xv[j] : ln_load4(xr, c, N, vx);
                f32x4 o = (v - mu) * r * ln_load4(gamma, c, N, vp) + ln_load4(beta, c, N, vp);
                if (mr != nullptr) o *= ln_load4(mr, c, N, vm);
                o *= out_scale;
                if (accumulate) o += ln_load4(yr, c, N, vy);
                ln_store4(yr, c, N, vy, o);
            }
        }
        for (int c = N + lane; c < N_pad; c += RP_WAVE) yr[c] = 0.f;
    }
}

// dn = dy_scale * dy [* mul], g = gamma * dn, nh = (x - mu) * r:
//   dx (+)= r * (g - mean(g) - nh * mean(g * nh));  dmul = dy_scale * dy * (gamma * nh + beta)
//   part[wave][0][:] = sum over the wave's rows of dn * nh,  part[wave][1][:] = sum of dn
template <int NV>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float *__restrict__ dy, int64_t lddy, float dy_scale,
                                                            const float *__restrict__ x, int64_t ldx,
                                                            const float *__restrict__ stats,
                                                            const float *__restrict__ gamma,
                                                            const float *__restrict__ beta,
                                                            const float *__restrict__ mul, int64_t ldmul, float *dx,
                                                            int64_t lddx, int N_pad, int accumulate,
                                                            float *__restrict__ dmul, int64_t lddmul,
                                                            float *__restrict__ part, int64_t M, int N, int vf) {
    const int lane = threadIdx.x & (RP_WAVE - 1);
    const int64_t w0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), W = (int64_t)gridDim.x * 4;
    if (w0 >= M) return;  // (whole waves leave: the partial rows of the waves that stay are the first min(W, M))
    const int nq = NV > 0 ? NV : (N + 255) / 256;
    const float invN = 1.f / (float)N;
    const bool vx = vf & LN_VX, vm = vf & LN_VMUL, vd = vf & LN_VY, vp = vf & LN_VP, vg = vf & LN_VDY, vdm = vf & LN_VDM;
    float *prow = part + w0 * 2 * (int64_t)N;
    f32x4 ag[NV > 0 ? NV : 1], ab[NV > 0 ? NV : 1];
#pragma unroll
    for (int j = 0; j < (NV > 0 ? NV : 1); ++j) {
        ag[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        ab[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    bool first = true;
    for (int64_t m = w0; m < M; m += W) {
        const float *xr = x + m * ldx, *gr = dy + m * lddy;
        const float *mr = mul != nullptr ? mul + m * ldmul : nullptr;
        float *dmr = mul != nullptr ? dmul + m * lddmul : nullptr;
        float *dxr = dx + m * lddx;
        const float mu = stats[2 * m], r = stats[2 * m + 1];
        f32x4 gv[NV > 0 ? NV : 1], nv[NV > 0 ? NV : 1];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < nq; ++j) {
            const int c = (j * RP_WAVE + lane) * 4;
            f32x4 g = {0.f, 0.f, 0.f, 0.f}, nh = {0.f, 0.f, 0.f, 0.f};
            if (c < N) {
                nh = (ln_load4(xr, c, N, vx) - mu) * r;
                const f32x4 gm = ln_load4(gamma, c, N, vp);
                f32x4 dn = ln_load4(gr, c, N, vg) * dy_scale;  // 0 in the columns that do not exist
                if (mr != nullptr) {
                    ln_store4(dmr, c, N, vdm, dn * (gm * nh + ln_load4(beta, c, N, vp)));
                    dn *= ln_load4(mr, c, N, vm);
                }
                g = gm * dn;
                s1 += ln_hsum(g);
                s2 += ln_hsum(g * nh);
                if (NV > 0) {
                    ag[j] += dn * nh;
                    ab[j] += dn;
                } else {  // the wave's own partial row, read and written by this lane alone
                    f32x4 pg = dn * nh, pb = dn;
                    if (!first) {
                        pg += ln_load4(prow, c, N, false);
                        pb += ln_load4(prow + N, c, N, false);
                    }
                    ln_store4(prow, c, N, false, pg);
                    ln_store4(prow + N, c, N, false, pb);
                }
            }
            if (NV > 0) {
                gv[j] = g;
                nv[j] = nh;
            }
        }
        first = false;
        s1 = rp_lane_sum(s1) * invN;
        s2 = rp_lane_sum(s2) * invN;
#pragma unroll
        for (int j = 0; j < nq; ++j) {
            const int c = (j * RP_WAVE + lane) * 4;
            if (c < N) {
                f32x4 g, nh;
                if (NV > 0) {
                    g = gv[j];
                    nh = nv[j];
                } else {
                    nh = (ln_load4(xr, c, N, vx) - mu) * r;
                    g = ln_load4(gamma, c, N, vp) * ln_load4(gr, c, N, vg) * dy_scale;
                    if (mr != nullptr) g *= ln_load4(mr, c, N, vm);
                }
                f32x4 o = (g - s1 - nh * s2) * r;
                if (accumulate) o += ln_load4(dxr, c, N, vd);
                ln_store4(dxr, c, N, vd, o);
            }
        }
        for (int c = N + lane; c < N_pad; c += RP_WAVE) dxr[c] = 0.f;
    }
    if (NV > 0) {
#pragma unroll
        for (int j = 0; j < nq; ++j) {
            const int c = (j * RP_WAVE + lane) * 4;
            ln_store4(prow, c, N, false, ag[j]);
            ln_store4(prow + N, c, N, false, ab[j]);
        }
    }
}

// 16 columns x 16 slices per block; slice s sums the partial rows s, s + 16, ...; the slices combine in order
__global__ __launch_bounds__(256) void layernorm_bwd_finish_kernel(const float *__restrict__ part, int nparts, int N,
                                                                   float *__restrict__ dgamma,
                                                                   float *__restrict__ dbeta) {
    __shared__ float red[2][256];
    const int c = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int n = blockIdx.x * 16 + c;
    float a = 0.f, b = 0.f;
    if (n < N) {
        for (int p = sl; p < nparts; p += 16) {
            a += part[(int64_t)p * 2 * N + n];
            b += part[((int64_t)p * 2 + 1) * N + n];
        }
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    if (sl == 0 && n < N) {
        for (int s = 1; s < 16; ++s) {
            a += red[0][s * 16 + c];
            b += red[1][s * 16 + c];
        }
        dgamma[n] = a;
        dbeta[n] = b;
    }
}

static bool ln_vec(const void *p, int64_t ld) { return p != nullptr && rp_aligned16(p) && ld % 4 == 0; }

// (one instance per 256 columns: a lane's registers are sized to the row, 1677 columns = 7 quads — at 8 the backward
// no longer fits two waves per SIMD and runs a third slower)
#define LN_DISPATCH(N, CALL)       \
    if ((N) <= 256) CALL(1);       \
    else if ((N) <= 512) CALL(2);  \
    else if ((N) <= 768) CALL(3);  \
    else if ((N) <= 1024) CALL(4); \
    else if ((N) <= 1280) CALL(5); \
    else if ((N) <= 1536) CALL(6); \
    else if ((N) <= 1792) CALL(7); \
    else if ((N) <= 2048) CALL(8); \
    else CALL(0)

extern "C" int rp_layernorm_fwd(const float *x, int64_t ldx, const float *gamma, const float *beta, float eps,
                                const float *mul, int64_t ldmul, float *y, int64_t ldy, int N_pad, float out_scale,
                                int accumulate, float *stats, int stats_given, int64_t M, int N, rp_stream_t stream) {
    RP_REQUIRE(x && gamma && beta && y, "layernorm_fwd: null pointer");
    RP_REQUIRE(M >= 0 && N >= 1 && N_pad >= N, "layernorm_fwd: bad M / N / N_pad");
    RP_REQUIRE(ldx >= N && ldy >= N_pad && (!mul || ldmul >= N), "layernorm_fwd: leading dimension too small");
    RP_REQUIRE(!stats_given || stats, "layernorm_fwd: stats_given without a statistics buffer");
    RP_REQUIRE(eps >= 0.f, "layernorm_fwd: negative eps");
    if (M == 0) return RP_OK;
    const int vf = (ln_vec(x, ldx) ? LN_VX : 0) | (ln_vec(mul, ldmul) ? LN_VMUL : 0) | (ln_vec(y, ldy) ? LN_VY : 0) |
                   ((rp_aligned16(gamma) && rp_aligned16(beta)) ? LN_VP : 0);
    int64_t blocks = rp_cdiv(M, 4);
    if (blocks > LN_FWD_BLOCKS) blocks = LN_FWD_BLOCKS;
    hipStream_t s = (hipStream_t)stream;
#define CALL(NV)                                                                                                      \
    hipLaunchKernelGGL((layernorm_fwd_kernel<NV>), dim3((unsigned)blocks), dim3(256), 0, s, x, ldx, gamma, beta, eps, \
                       mul, ldmul, y, ldy, N_pad, out_scale, accumulate, stats, stats_given, M, N, vf)
    LN_DISPATCH(N, CALL);
#undef CALL
    RP_LAUNCH_CHECK("layernorm_fwd");
    return RP_OK;
}

extern "C" int rp_layernorm_bwd_workspace_bytes(int N, size_t *bytes) {
    RP_REQUIRE(bytes && N >= 1, "layernorm_bwd_workspace_bytes: bad argument");
    *bytes = (size_t)LN_BWD_BLOCKS * 4 * 2 * (size_t)N * sizeof(float) + 256;
    return RP_OK;
}

extern "C" int rp_layernorm_bwd(const float *dy, int64_t lddy, float dy_scale, const float *x, int64_t ldx,
                                const float *stats, const float *gamma, const float *beta, const float *mul,
                                int64_t ldmul, float *dx, int64_t lddx, int N_pad, int accumulate, float *dmul,
                                int64_t lddmul, float *dgamma, float *dbeta, int64_t M, int N, void *workspace,
                                size_t workspace_bytes, rp_stream_t stream) {
    RP_REQUIRE(dy && x && stats && gamma && beta && dx && dgamma && dbeta && workspace, "layernorm_bwd: null pointer");
    RP_REQUIRE(M >= 1 && N >= 1 && N_pad >= N, "layernorm_bwd: bad M / N / N_pad");
    RP_REQUIRE(lddy >= N && ldx >= N && lddx >= N_pad, "layernorm_bwd: leading dimension too small");
    RP_REQUIRE(!mul || (dmul && ldmul >= N && lddmul >= N), "layernorm_bwd: mul needs dmul, both at least N wide");
    size_t need = 0;
    rp_layernorm_bwd_workspace_bytes(N, &need);
    RP_REQUIRE(workspace_bytes >= need, "layernorm_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    float *part = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    const int vf = (ln_vec(x, ldx) ? LN_VX : 0) | (ln_vec(mul, ldmul) ? LN_VMUL : 0) | (ln_vec(dx, lddx) ? LN_VY : 0) |
                   ((rp_aligned16(gamma) && rp_aligned16(beta)) ? LN_VP : 0) | (ln_vec(dy, lddy) ? LN_VDY : 0) |
                   (ln_vec(dmul, lddmul) ? LN_VDM : 0);
    int64_t blocks = rp_cdiv(M, 4);
    if (blocks > LN_BWD_BLOCKS) blocks = LN_BWD_BLOCKS;
    const int nparts = (int)(M < blocks * 4 ? M : blocks * 4);
    hipStream_t s = (hipStream_t)stream;
#define CALL(NV)                                                                                                         \
    hipLaunchKernelGGL((layernorm_bwd_kernel<NV>), dim3((unsigned)blocks), dim3(256), 0, s, dy, lddy, dy_scale, x, ldx, \
                       stats, gamma, beta, mul, ldmul, dx, lddx, N_pad, accumulate, dmul, lddmul, part, M, N, vf)
    LN_DISPATCH(N, CALL);
#undef CALL
    RP_LAUNCH_CHECK("layernorm_bwd");
    hipLaunchKernelGGL(layernorm_bwd_finish_kernel, dim3((unsigned)rp_cdiv(N, 16)), dim3(256), 0, s, part, nparts, N,
                       dgamma, dbeta);
    RP_LAUNCH_CHECK("layernorm_bwd (finish)");
    return RP_OK;
}
