// Two-task loss heads whose tasks are coupled, forward and backward, gfx950.
//   mode RP_PAIR_ESSM (0)  multi_task/essm.py:69-75   loss = BCE(p1 p2, y2) + w BCE(p1, y1)
//   mode RP_PAIR_AITM (1)  multi_task/aitm.py:84-100  loss = BCE(p1, y1) + BCE(p2, y2) + c sum_b max(p2 - p1, 0)
// with p = sigmoid(z) (apply_sigmoid) or p = z, BCE the mean over the batch as ATen forms it (logs clamped at -100, the
// backward's denominator at 1e-12: loss.hip).  rp_sigmoid_bce_* adds independent per-task terms only; here the product and
// the constraint need both tasks' probabilities of a row at once.
//
// One pass over [B], a few bytes per sample, like loss.hip: the point is one launch plus a one-block finish instead of
// the reference's ~12 ATen launches, and a fixed summation order.  Every workgroup writes THREE partial sums (planes of
// rp_loss_partials(B) floats): the two BCE sums and the constraint sum.  The finish adds each plane in a fixed order and only
// then scales (1/B for the means, the coefficient for the terms the reference scales) and combines them with the
// reference's own fp32 additions.  No atomics: the loss is bit-identical from run to run.
#include "common.h"

#define PL_BLOCK 256

__device__ __forceinline__ float pl_bce(float p, float y) {
    return -(y * fmaxf(logf(p), -100.f) + (1.f - y) * fmaxf(log1pf(-p), -100.f));
}
// ATen binary_cross_entropy_backward without the incoming gradient: (p - y) / max((1 - p) p, 1e-12)
__device__ __forceinline__ float pl_dbce(float p, float y) { return (p - y) / fmaxf((1.f - p) * p, 1e-12f); }

__global__ __launch_bounds__(PL_BLOCK) void pair_loss_fwd_kernel(const float *__restrict__ z1, const float *__restrict__ z2,
                                                                  const float *__restrict__ y1, const float *__restrict__ y2,
                                                                  int64_t B, int mode, int apply_sigmoid,
                                                                  float *__restrict__ p1o, float *__restrict__ p2o,
                                                                  float *__restrict__ partial) {
    __shared__ float sh[4];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int64_t b = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x; b < B; b += (int64_t)gridDim.x * PL_BLOCK) {
        const float a1 = z1[b], a2 = z2[b];
        const float p1 = apply_sigmoid ? rp_sigmoid(a1) : a1;
        const float p2 = apply_sigmoid ? rp_sigmoid(a2) : a2;
        p1o[b] = p1;
        p2o[b] = p2;
        if (mode == RP_PAIR_ESSM) {
            s0 += pl_bce(__fmul_rn(p1, p2), y2[b]);
            s1 += pl_bce(p1, y1[b]);
        } else {
            s0 += pl_bce(p1, y1[b]);
            s1 += pl_bce(p2, y2[b]);
            s2 += fmaxf(__fsub_rn(p2, p1), 0.f);
        }
    }
    const int nb = gridDim.x;
    const float t0 = rp_block_sum_256(s0, sh), t1 = rp_block_sum_256(s1, sh), t2 = rp_block_sum_256(s2, sh);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = t0;
        partial[nb + blockIdx.x] = t1;
        partial[2 * nb + blockIdx.x] = t2;
    }
}

// (no contraction into fmas: the reference rounds each mean and each product before it adds)
__global__ __launch_bounds__(PL_BLOCK) void pair_loss_finish_kernel(const float *__restrict__ partial, int nb, int mode,
                                                                     float coef, float inv_b, float *__restrict__ loss) {
    __shared__ float sh[4];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < nb; i += PL_BLOCK) {
        s0 += partial[i];
        s1 += partial[nb + i];
        s2 += partial[2 * nb + i];
    }
    const float t0 = rp_block_sum_256(s0, sh), t1 = rp_block_sum_256(s1, sh), t2 = rp_block_sum_256(s2, sh);
    if (threadIdx.x == 0) {
        const float m0 = __fmul_rn(t0, inv_b), m1 = __fmul_rn(t1, inv_b);
        loss[0] = mode == RP_PAIR_ESSM ? __fadd_rn(m0, __fmul_rn(coef, m1))
                                       : __fadd_rn(__fadd_rn(m0, m1), __fmul_rn(coef, t2));
    }
}

__global__ __launch_bounds__(PL_BLOCK) void pair_loss_bwd_kernel(const float *__restrict__ p1i, const float *__restrict__ p2i,
                                                                  const float *__restrict__ y1, const float *__restrict__ y2,
                                                                  const float *__restrict__ gloss, int64_t B, int mode,
                                                                  float coef, float inv_b, int apply_sigmoid,
                                                                  float *__restrict__ dz1, float *__restrict__ dz2) {
    const float g = gloss[0], gm = g * inv_b;  // the gradient of each mean
    for (int64_t b = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x; b < B; b += (int64_t)gridDim.x * PL_BLOCK) {
        const float p1 = p1i[b], p2 = p2i[b];
        float d1, d2;
        if (mode == RP_PAIR_ESSM) {
            const float dq = pl_dbce(__fmul_rn(p1, p2), y2[b]) * gm;
            d1 = dq * p2 + coef * (pl_dbce(p1, y1[b]) * gm);
            d2 = dq * p1;
        } else {
            // ATen's maximum backward: the gradient goes to the larger argument, half of it to each at a tie
            const float s = p2 > p1 ? 1.f : (p2 < p1 ? 0.f : 0.5f);
            const float gc = coef * g * s;
            d1 = pl_dbce(p1, y1[b]) * gm - gc;
            d2 = pl_dbce(p2, y2[b]) * gm + gc;
        }
        if (apply_sigmoid) {
            d1 *= p1 * (1.f - p1);
            d2 *= p2 * (1.f - p2);
        }
        dz1[b] = d1;
        dz2[b] = d2;
    }
}

static int pl_blocks(int64_t B) { return rp_loss_partials(B); }

extern "C" int rp_pair_loss_fwd(const float *z1, const float *z2, const float *y1, const float *y2, int64_t B, int mode,
                                float coef, int apply_sigmoid, float *p1, float *p2, float *partial, float *loss,
                                rp_stream_t stream) {
    RP_REQUIRE(z1 && z2 && y1 && y2 && p1 && p2 && partial && loss, "pair_loss_fwd: null pointer");
    RP_REQUIRE(B >= 1, "pair_loss_fwd: empty batch");
    RP_REQUIRE(mode == RP_PAIR_ESSM || mode == RP_PAIR_AITM, "pair_loss_fwd: mode %d is neither RP_PAIR_ESSM nor RP_PAIR_AITM", mode);
    const int nb = pl_blocks(B);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pair_loss_fwd_kernel, dim3(nb), dim3(PL_BLOCK), 0, s, z1, z2, y1, y2, B, mode, apply_sigmoid, p1, p2,
                       partial);
    RP_LAUNCH_CHECK("pair_loss_fwd");
    hipLaunchKernelGGL(pair_loss_finish_kernel, dim3(1), dim3(PL_BLOCK), 0, s, partial, nb, mode, coef, 1.f / (float)B, loss);
    RP_LAUNCH_CHECK("pair_loss_finish");
    return RP_OK;
}

extern "C" int rp_pair_loss_bwd(const float *p1, const float *p2, const float *y1, const float *y2, const float *gloss,
                                int64_t B, int mode, float coef, int apply_sigmoid, float *dz1, float *dz2,
                                rp_stream_t stream) {
    RP_REQUIRE(p1 && p2 && y1 && y2 && gloss && dz1 && dz2, "pair_loss_bwd: null pointer");
    RP_REQUIRE(B >= 1, "pair_loss_bwd: empty batch");
    RP_REQUIRE(mode == RP_PAIR_ESSM || mode == RP_PAIR_AITM, "pair_loss_bwd: mode %d is neither RP_PAIR_ESSM nor RP_PAIR_AITM", mode);
    hipLaunchKernelGGL(pair_loss_bwd_kernel, dim3(pl_blocks(B)), dim3(PL_BLOCK), 0, (hipStream_t)stream, p1, p2, y1, y2, gloss,
                       B, mode, coef, 1.f / (float)B, apply_sigmoid, dz1, dz2);
    RP_LAUNCH_CHECK("pair_loss_bwd");
    return RP_OK;
}
