// NARM's attention readout (rec_pangu/models/sequence/narm.py:52-61), gfx950:
//   alpha[b, l] = sum_h v[h] m[b, l] sigmoid(q1[b, l, h] + q2[b, h]),   m = (ids[b, l] > 0)
//   out[b]      = [ sum_l alpha[b, l] G[b, l, :] , ht[b, :] ]            (width 2H)
// One wave per batch row, lane c owns the columns c and c + 64 (H <= 128); the sum over h is a butterfly in a fixed order,
// the sum over l runs in position order.  No [B, L, H] intermediate: the forward keeps alpha [B, L] only, the backward
// recomputes the sigmoid.  dv: per-workgroup slabs (at most NARM_SLABS) added in workgroup order by a second launch.
#include "common.h"

namespace {

constexpr int NARM_MAX_H = 128;
constexpr int NARM_SLABS = 1024;

__global__ __launch_bounds__(256) void narm_attn_fwd_kernel(const float *__restrict__ q1, const float *__restrict__ q2,
                                                            const float *__restrict__ v, const int64_t *__restrict__ ids,
                                                            const float *__restrict__ G, const float *__restrict__ ht, int64_t B,
                                                            int64_t L, int H, float *__restrict__ alpha,
                                                            float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int c0 = lane, c1 = lane + 64;
    const bool u0 = c0 < H, u1 = c1 < H;
    const float v0 = u0 ? v[c0] : 0.f, v1 = u1 ? v[c1] : 0.f;
    const float p0 = u0 ? q2[b * H + c0] : 0.f, p1 = u1 ? q2[b * H + c1] : 0.f;
    float a0 = 0.f, a1 = 0.f;
    for (int64_t l = 0; l < L; ++l) {
        const int64_t row = b * L + l;
        float al = 0.f;
        if (ids[row] > 0) {  // (uniform over the wave)
            float s = 0.f;
            if (u0) s += v0 * rp_sigmoid(q1[row * H + c0] + p0);
            if (u1) s += v1 * rp_sigmoid(q1[row * H + c1] + p1);
            al = rp_lane_sum(s);
        }
        if (lane == 0) alpha[row] = al;
        if (u0) a0 += al * G[row * H + c0];
        if (u1) a1 += al * G[row * H + c1];
    }
    float *o = out + b * 2 * H;
    if (u0) o[c0] = a0, o[H + c0] = ht[b * H + c0];
    if (u1) o[c1] = a1, o[H + c1] = ht[b * H + c1];
}

// dout [B, 2H] -> dq1 [B, L, H], dq2 [B, H], dG [B, L, H], dht [B, H], dv slabs [gridDim.x][H]
__global__ __launch_bounds__(256) void narm_attn_bwd_kernel(const float *__restrict__ q1, const float *__restrict__ q2,
                                                            const float *__restrict__ v, const int64_t *__restrict__ ids,
                                                            const float *__restrict__ G, const float *__restrict__ alpha,
                                                            const float *__restrict__ dout, int64_t B, int64_t L, int H,
                                                            float *__restrict__ dq1, float *__restrict__ dq2,
                                                            float *__restrict__ dG, float *__restrict__ dht,
                                                            float *__restrict__ slab) {
    __shared__ float part[4][NARM_MAX_H];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c0 = lane, c1 = lane + 64;
    const bool u0 = c0 < H, u1 = c1 < H;
    const float v0 = u0 ? v[c0] : 0.f, v1 = u1 ? v[c1] : 0.f;
    float dv0 = 0.f, dv1 = 0.f;
    for (int64_t b = (int64_t)blockIdx.x * 4 + w; b < B; b += (int64_t)gridDim.x * 4) {
        const float p0 = u0 ? q2[b * H + c0] : 0.f, p1 = u1 ? q2[b * H + c1] : 0.f;
        const float g0 = u0 ? dout[b * 2 * H + c0] : 0.f, g1 = u1 ? dout[b * 2 * H + c1] : 0.f;
        float d20 = 0.f, d21 = 0.f;
        for (int64_t l = 0; l < L; ++l) {
            const int64_t row = b * L + l;
            const float al = alpha[row];
            float s = 0.f;
            if (u0) s += g0 * G[row * H + c0];
            if (u1) s += g1 * G[row * H + c1];
            const float ds = ids[row] > 0 ? rp_lane_sum(s) : 0.f;  // d alpha through the mask
            if (u0) {
                const float sg = rp_sigmoid(q1[row * H + c0] + p0), d = ds * v0 * sg * (1.f - sg);
                dq1[row * H + c0] = d, d20 += d, dv0 += ds * sg, dG[row * H + c0] = al * g0;
            }
            if (u1) {
                const float sg = rp_sigmoid(q1[row * H + c1] + p1), d = ds * v1 * sg * (1.f - sg);
                dq1[row * H + c1] = d, d21 += d, dv1 += ds * sg, dG[row * H + c1] = al * g1;
            }
        }
        if (u0) dq2[b * H + c0] = d20, dht[b * H + c0] = dout[b * 2 * H + H + c0];
        if (u1) dq2[b * H + c1] = d21, dht[b * H + c1] = dout[b * 2 * H + H + c1];
    }
    if (u0) part[w][c0] = dv0;
    if (u1) part[w][c1] = dv1;
    __syncthreads();
    for (int c = threadIdx.x; c < H; c += 256)
        slab[(int64_t)blockIdx.x * H + c] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

__global__ __launch_bounds__(256) void narm_dv_finish_kernel(const float *__restrict__ slab, int nslab, int H,
                                                             float *__restrict__ dv) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= H) return;
    float s = 0.f;
    for (int q = 0; q < nslab; ++q) s += slab[(int64_t)q * H + c];
    dv[c] = s;
}

int narm_slabs(int64_t B) {
    const int64_t n = rp_cdiv(B, 4);
    return (int)(n < NARM_SLABS ? n : NARM_SLABS);
}

}  // namespace

extern "C" int rp_narm_attn_workspace_bytes(int64_t B, int H, size_t *bytes) {
    RP_REQUIRE(bytes && B >= 0 && H >= 1 && H <= NARM_MAX_H, "narm_attn_workspace_bytes: need B >= 0 and 1 <= H <= %d", NARM_MAX_H);
    *bytes = sizeof(float) * (size_t)H * (size_t)(B > 0 ? narm_slabs(B) : 1);
    return RP_OK;
}

extern "C" int rp_narm_attn_fwd(const float *q1, const float *q2, const float *v, const int64_t *ids, const float *G,
                                const float *ht, int64_t B, int64_t L, int H, float *alpha, float *out, rp_stream_t stream) {
    RP_REQUIRE(q1 && q2 && v && ids && G && ht && alpha && out, "narm_attn_fwd: null pointer");
    RP_REQUIRE(B >= 0 && L >= 1 && H >= 1 && H <= NARM_MAX_H, "narm_attn_fwd: need B >= 0, L >= 1 and 1 <= H <= %d", NARM_MAX_H);
    if (B == 0) return RP_OK;
    hipLaunchKernelGGL(narm_attn_fwd_kernel, dim3((unsigned)rp_cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, q1, q2, v, ids,
                       G, ht, B, L, H, alpha, out);
    RP_LAUNCH_CHECK("narm_attn_fwd");
    return RP_OK;
}

extern "C" int rp_narm_attn_bwd(const float *q1, const float *q2, const float *v, const int64_t *ids, const float *G,
                                const float *alpha, const float *dout, int64_t B, int64_t L, int H, float *dq1, float *dq2,
                                float *dG, float *dht, float *dv, void *workspace, size_t workspace_bytes,
                                rp_stream_t stream) {
    RP_REQUIRE(q1 && q2 && v && ids && G && alpha && dout && dq1 && dq2 && dG && dht && dv && workspace,
               "narm_attn_bwd: null pointer");
    RP_REQUIRE(B >= 0 && L >= 1 && H >= 1 && H <= NARM_MAX_H, "narm_attn_bwd: need B >= 0, L >= 1 and 1 <= H <= %d", NARM_MAX_H);
    const int nslab = B > 0 ? narm_slabs(B) : 0;
    RP_REQUIRE(workspace_bytes >= sizeof(float) * (size_t)H * (size_t)(nslab ? nslab : 1), "narm_attn_bwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float *slab = static_cast<float *>(workspace);
    if (B > 0) {
        hipLaunchKernelGGL(narm_attn_bwd_kernel, dim3((unsigned)nslab), dim3(256), 0, s, q1, q2, v, ids, G, alpha, dout, B, L, H,
                           dq1, dq2, dG, dht, slab);
        RP_LAUNCH_CHECK("narm_attn_bwd");
    }
    hipLaunchKernelGGL(narm_dv_finish_kernel, dim3((unsigned)rp_cdiv(H, 256)), dim3(256), 0, s, (const float *)slab, nslab, H, dv);
    RP_LAUNCH_CHECK("narm_attn_bwd (dv)");
    return RP_OK;
}
