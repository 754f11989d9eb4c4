// Temporal warp for TC-Stereo on gfx950: pose-based forward warp of the previous frame's disparity
// and features (softmax splatting), backward grid, hidden-state sampling.
// Replaces core/utils/geo_utils.py (warp, get_backward_grid) and the CuPy kernel softsplat_out
// (core/utils/splatting/softsplat.py:285-335) of the reference.
//
// Splat design: one thread per SOURCE pixel and channel group.  Lanes are horizontally adjacent
// source pixels, which for a rigid camera motion land on horizontally adjacent targets, so each
// atomic wave-instruction covers ~256 contiguous bytes of one NCHW channel plane — the shape the
// memory-side f32 atomics of MI355X run fastest on.  Geometry (flow, weights, exp(metric)) is
// computed once per thread, not once per (channel, pixel) as the reference kernel does.
// The opt-in ordered splat (k_ord_*, below) sums the same contributions per target in ascending source order: bit-reproducible.
#include "tcs_common.h"

struct Cam {
    float K[9], Ki[9], T[12], bf;
};

__device__ __forceinline__ Cam load_cam(const float* __restrict__ T_rel, const float* __restrict__ K,
                                        const float* __restrict__ K_inv, const float* __restrict__ baseline, int b) {
    Cam c;
#pragma unroll
    for (int i = 0; i < 9; ++i) { c.K[i] = K[b * 9 + i]; c.Ki[i] = K_inv[b * 9 + i]; }
#pragma unroll
    for (int i = 0; i < 12; ++i) c.T[i] = T_rel[b * 16 + i];
    c.bf = baseline[b] * c.K[0];
    return c;
}

__device__ __forceinline__ float fix_nonfinite(float v) { return isfinite(v) ? v : -1.0f; }

// disparity at (x,y) -> 3-D point -> rigid transform -> (new depth, projected pixel)
__device__ __forceinline__ void reproject(const Cam& c, float disp, float x, float y, float& zp, float& u, float& v) {
    const float depth = c.bf / fmaxf(disp, 0.001f);                       // disp2depth, geo_utils.py:16
    const float rx = c.Ki[0] * x + c.Ki[1] * y + c.Ki[2];                 // pixel2point, geo_utils.py:41
    const float ry = c.Ki[3] * x + c.Ki[4] * y + c.Ki[5];
    const float rz = c.Ki[6] * x + c.Ki[7] * y + c.Ki[8];
    const float px = depth * rx, py = depth * ry, pz = depth * rz;
    const float qx = c.T[0] * px + c.T[1] * py + c.T[2] * pz + c.T[3];    // relative_transform, geo_utils.py:144
    const float qy = c.T[4] * px + c.T[5] * py + c.T[6] * pz + c.T[7];
    const float qz = c.T[8] * px + c.T[9] * py + c.T[10] * pz + c.T[11];
    zp = qz;
    u = fix_nonfinite((c.K[0] * qx + c.K[1] * qy + c.K[2] * qz) / qz);    // point2pixel, geo_utils.py:55-56
    v = fix_nonfinite((c.K[3] * qx + c.K[4] * qy + c.K[5] * qz) / qz);
}

// ------------------------------------------------------------------------------------------------
// forward geometry: new disparity, validity, forward flow, per-block partial sums of the disparity
// ------------------------------------------------------------------------------------------------
// MIXED (the *_mixed entry points): a batch element with start[b] != 0 begins a sequence.  It reads none of its inputs, writes
// cur_disp = valid = flow = 0 (valid = 0: the splats skip it, atomic and ordered alike) and leaves exact zeros in its block partials.
// The start branch leaves the kernel first (block-uniform), so that the code after it is the non-mixed kernel's, contraction included.
template <bool MIXED>
__device__ __forceinline__ void warp_geometry_body(const float* __restrict__ disp, const float* __restrict__ T_rel,
                                                   const float* __restrict__ K, const float* __restrict__ K_inv,
                                                   const float* __restrict__ baseline, const unsigned char* __restrict__ start,
                                                   int H, int W, float* __restrict__ cur_disp, float* __restrict__ valid,
                                                   float* __restrict__ flow, float* __restrict__ partial) {
    __shared__ float red[4];
    const int b = blockIdx.y, HW = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (MIXED && start[b]) {
        if (p < HW) {
            cur_disp[(size_t)b * HW + p] = 0.f;
            valid[(size_t)b * HW + p] = 0.f;
            flow[((size_t)b * 2 + 0) * HW + p] = 0.f;
            flow[((size_t)b * 2 + 1) * HW + p] = 0.f;
        }
        if (threadIdx.x == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = 0.f;
        return;
    }
    float cd = 0.f;
    if (p < HW) {
        const Cam c = load_cam(T_rel, K, K_inv, baseline, b);
        const int y = p / W, x = p - y * W;
        float zp, u, v;
        reproject(c, disp[(size_t)b * HW + p], (float)x, (float)y, zp, u, v);
        cd = fix_nonfinite(c.bf / zp);                                     // depth2disp, geo_utils.py:27-28
        cur_disp[(size_t)b * HW + p] = cd;
        valid[(size_t)b * HW + p] = (cd > 0.f && cd < (float)W) ? 1.f : 0.f;   // geo_utils.py:186
        flow[((size_t)b * 2 + 0) * HW + p] = u - (float)x;                 // geo_utils.py:192
        flow[((size_t)b * 2 + 1) * HW + p] = v - (float)y;
    }
    const float s = wave_sum(cd);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void k_warp_geometry(const float* __restrict__ disp, const float* __restrict__ T_rel,
                                                       const float* __restrict__ K, const float* __restrict__ K_inv,
                                                       const float* __restrict__ baseline, int H, int W,
                                                       float* __restrict__ cur_disp, float* __restrict__ valid,
                                                       float* __restrict__ flow, float* __restrict__ partial) {
    warp_geometry_body<false>(disp, T_rel, K, K_inv, baseline, nullptr, H, W, cur_disp, valid, flow, partial);
}

__global__ __launch_bounds__(256) void k_warp_geometry_mixed(const float* __restrict__ disp, const float* __restrict__ T_rel,
                                                             const float* __restrict__ K, const float* __restrict__ K_inv,
                                                             const float* __restrict__ baseline, const unsigned char* __restrict__ start,
                                                             int H, int W, float* __restrict__ cur_disp, float* __restrict__ valid,
                                                             float* __restrict__ flow, float* __restrict__ partial) {
    warp_geometry_body<true>(disp, T_rel, K, K_inv, baseline, start, H, W, cur_disp, valid, flow, partial);
}

// fixed-order reduction of the partial sums (the total is valid in thread 0)
__device__ __forceinline__ float partial_total(const float* __restrict__ partial, int n) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// -> mean over ALL pixels of the batch (geo_utils.py:193)
__global__ __launch_bounds__(256) void k_mean(const float* __restrict__ partial, int n, float inv_count, float* __restrict__ mean) {
    const float t = partial_total(partial, n);
    if (threadIdx.x == 0) *mean = t * inv_count;
}

// -> mean over the pixels of the temporal elements (start[b] == 0) only: the reference's warp() on that sub-batch.  The reciprocal is
// formed as the host forms k_mean's; without a temporal element the mean is 0 (no 0/0; nothing reads it then).
__global__ __launch_bounds__(256) void k_mean_mixed(const float* __restrict__ partial, int n, const unsigned char* __restrict__ start, int B,
                                                    long long HW, float* __restrict__ mean) {
    const float t = partial_total(partial, n);
    if (threadIdx.x == 0) {
        long long count = 0;
        for (int b = 0; b < B; ++b) count += start[b] ? 0 : HW;
        *mean = count > 0 ? t * (1.0f / (float)count) : 0.f;
    }
}

__global__ __launch_bounds__(256) void k_metric(const float* __restrict__ cur_disp, const float* __restrict__ mean, int n,
                                                float* __restrict__ metric) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) metric[i] = fminf(fmaxf(cur_disp[i] - *mean, -50.f), 50.f);
}

// ------------------------------------------------------------------------------------------------
// splat.  MODE 0: plain summation splat of `in` (softsplat_func.forward, softsplat.py:285-335).
//         MODE 1: warp(): channels [0,C) are prev_fmap, channel C the new disparity, channel C+1 the
//                 normaliser; every value is scaled by valid*exp(metric) (softsplat.py:236,250).
// ------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void k_splat(const float* __restrict__ in, const float* __restrict__ flow,
                                               const float* __restrict__ cur_disp, const float* __restrict__ valid,
                                               const float* __restrict__ mean, int C, int H, int W, int ch_per_group,
                                               float* __restrict__ out) {
    const int b = blockIdx.y, HW = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    const float fx = (float)x + flow[((size_t)b * 2 + 0) * HW + p];
    const float fy = (float)y + flow[((size_t)b * 2 + 1) * HW + p];
    if (!isfinite(fx) || !isfinite(fy)) return;                            // softsplat.py:301-302
    float scale = 1.f, cd = 0.f;
    if (MODE == 1) {
        if (valid[(size_t)b * HW + p] == 0.f) return;                      // contributes exact zeros
        cd = cur_disp[(size_t)b * HW + p];
        scale = expf(fminf(fmaxf(cd - *mean, -50.f), 50.f));               // geo_utils.py:193, softsplat.py:250
    }
    const float x0f = floorf(fx), y0f = floorf(fy);
    if (!(x0f >= -2.f && x0f <= (float)W && y0f >= -2.f && y0f <= (float)H)) return;   // every corner out of frame
    const int x0 = (int)x0f, y0 = (int)y0f;
    // corner weights exactly as softsplat.py:315-318
    const float wnw = ((float)(x0 + 1) - fx) * ((float)(y0 + 1) - fy);
    const float wne = (fx - (float)x0) * ((float)(y0 + 1) - fy);
    const float wsw = ((float)(x0 + 1) - fx) * (fy - (float)y0);
    const float wse = (fx - (float)x0) * (fy - (float)y0);
    const bool xl = x0 >= 0 && x0 < W, xr = x0 + 1 >= 0 && x0 + 1 < W;
    const bool yt = y0 >= 0 && y0 < H, yb = y0 + 1 >= 0 && y0 + 1 < H;
    const int tnw = y0 * W + x0;
    const int Ctot = (MODE == 1) ? C + 2 : C;
    const int c_lo = blockIdx.z * ch_per_group, c_hi = min(Ctot, c_lo + ch_per_group);
    float* ob = out + (size_t)b * Ctot * HW;
    for (int c = c_lo; c < c_hi; ++c) {
        float v;
        if (MODE == 1) v = (c < C) ? in[((size_t)b * C + c) * HW + p] * scale : (c == C ? cd * scale : scale);
        else v = in[((size_t)b * C + c) * HW + p];
        float* o = ob + (size_t)c * HW + tnw;
        if (xl && yt) unsafeAtomicAdd(o, v * wnw);
        if (xr && yt) unsafeAtomicAdd(o + 1, v * wne);
        if (xl && yb) unsafeAtomicAdd(o + W, v * wsw);
        if (xr && yb) unsafeAtomicAdd(o + W + 1, v * wse);
    }
}

// explicit zero fill of the splat accumulator.  (A captured hipMemsetAsync node did not re-clear the
// 20 MB accumulator on HIP-graph replays on ROCm 7.2: the second replay of a frame summed into the previous
// frame's values.  A kernel node has no such ambiguity.)
__global__ __launch_bounds__(256) void k_zero_fill(float4* __restrict__ p, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// normalise (softsplat.py:257-270, 'clipeps'), split, and the temporal cost (tc_stereo.py:139-140)
// One block = 64 consecutive pixels x 4 channel quarters (one wave each: coalesced rows of 64 floats per channel); the
// three sums of the cosine are combined across the quarters through LDS in a fixed order (deterministic).
// A start element of a mixed batch (start[b] != 0) reads neither the accumulator nor cur_fmap: its disparity, mask and cost are the
// first-frame prior (tcs_corr_build's sparse_*), its warped features 0.  Block-uniform: the whole block returns before the barrier.
template <bool MIXED>
__device__ __forceinline__ bool finish_start(const unsigned char* __restrict__ start, const float* __restrict__ prior_disp,
                                             const float* __restrict__ prior_cost, const float* __restrict__ prior_mask, int C, int HW,
                                             float* __restrict__ out_disp, float* __restrict__ out_fmap, float* __restrict__ out_mask,
                                             float* __restrict__ out_cost) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    if (!MIXED || !start[b]) return false;
    const int p = blockIdx.x * 64 + lane;
    if (p >= HW) return true;
    const size_t i = (size_t)b * HW + p;
    if (q == 0) {
        out_disp[i] = prior_disp[i];
        out_mask[i] = prior_mask[i];
        if (out_cost) out_cost[i] = prior_cost[i];
    }
    if (out_fmap) {
        const int cq = (C + 3) / 4, c_lo = q * cq, c_hi = min(C, c_lo + cq);
        for (int c = c_lo; c < c_hi; ++c) out_fmap[((size_t)b * C + c) * HW + p] = 0.f;
    }
    return true;
}

template <bool MIXED>
__device__ __forceinline__ void warp_finish_body(const float* __restrict__ acc, const float* __restrict__ cur_fmap,
                                                 const unsigned char* __restrict__ start, const float* __restrict__ prior_disp,
                                                 const float* __restrict__ prior_cost, const float* __restrict__ prior_mask,
                                                 int C, int HW, float* __restrict__ out_disp, float* __restrict__ out_fmap,
                                                 float* __restrict__ out_mask, float* __restrict__ out_cost) {
    __shared__ float s_part[3][4][64];
    if (finish_start<MIXED>(start, prior_disp, prior_cost, prior_mask, C, HW, out_disp, out_fmap, out_mask, out_cost)) return;
    const int b = blockIdx.y, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int p_raw = blockIdx.x * 64 + lane;
    const bool active = p_raw < HW;
    const int p = active ? p_raw : HW - 1;
    const float* a = acc + (size_t)b * (C + 2) * HW + p;
    const float norm = a[(size_t)(C + 1) * HW];
    const float mask = (norm != 0.f) ? 1.f : 0.f;
    const float den = fmaxf(norm, 1e-7f);
    if (q == 0 && active) {
        out_disp[(size_t)b * HW + p] = a[(size_t)C * HW] / den;
        out_mask[(size_t)b * HW + p] = mask;
    }
    const int cq = (C + 3) / 4, c_lo = q * cq, c_hi = min(C, c_lo + cq);
    float dot = 0.f, n1 = 0.f, nw = 0.f;
    for (int c = c_lo; c < c_hi; ++c) {
        const float fw = a[(size_t)c * HW] / den;
        if (out_fmap && active) out_fmap[((size_t)b * C + c) * HW + p] = fw;
        if (out_cost) {
            const float f1 = cur_fmap[((size_t)b * C + c) * HW + p];
            dot = fmaf(f1, fw, dot);
            n1 = fmaf(f1, f1, n1);
            nw = fmaf(fw, fw, nw);
        }
    }
    if (!out_cost) return;
    s_part[0][q][lane] = dot; s_part[1][q][lane] = n1; s_part[2][q][lane] = nw;
    __syncthreads();
    if (q == 0 && active) {
        float t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = ((s_part[k][0][lane] + s_part[k][1][lane]) + s_part[k][2][lane]) + s_part[k][3][lane];
        out_cost[(size_t)b * HW + p] = t[0] / (fmaxf(sqrtf(t[1]), 1e-12f) * fmaxf(sqrtf(t[2]), 1e-12f)) * mask;
    }
}

__global__ __launch_bounds__(256) void k_warp_finish(const float* __restrict__ acc, const float* __restrict__ cur_fmap,
                                                     int C, int HW, float* __restrict__ out_disp, float* __restrict__ out_fmap,
                                                     float* __restrict__ out_mask, float* __restrict__ out_cost) {
    warp_finish_body<false>(acc, cur_fmap, nullptr, nullptr, nullptr, nullptr, C, HW, out_disp, out_fmap, out_mask, out_cost);
}

__global__ __launch_bounds__(256) void k_warp_finish_mixed(const float* __restrict__ acc, const float* __restrict__ cur_fmap,
                                                           const unsigned char* __restrict__ start, const float* __restrict__ prior_disp,
                                                           const float* __restrict__ prior_cost, const float* __restrict__ prior_mask,
                                                           int C, int HW, float* __restrict__ out_disp, float* __restrict__ out_fmap,
                                                           float* __restrict__ out_mask, float* __restrict__ out_cost) {
    warp_finish_body<true>(acc, cur_fmap, start, prior_disp, prior_cost, prior_mask, C, HW, out_disp, out_fmap, out_mask, out_cost);
}

// ------------------------------------------------------------------------------------------------
// Ordered splat (tcs_warp_forward_ordered, tcs_softsplat_sum_ordered): the same contributions as k_splat, summed per target in
// ascending source-pixel order with plain fp32 adds, so the result does not depend on scheduling.  Inverted index per batch element:
//   count  (integer atomics: contributions per target)  ->  scan (exclusive prefix sum: bucket offsets)  ->  place (each in-frame
//   corner once into its target's bucket, atomic cursor)  ->  rank (each entry moves to start + #entries of its bucket with a smaller
//   source index: the bucket is now sorted; sources are distinct within a bucket)  ->  gather (one lane per target sums its bucket).
// Bucket entries carry the corner weight computed exactly as k_splat computes it.  A bucket is summed by one lane (per channel
// quarter), so its time is linear in its length: real motion puts 1-4 entries in a bucket; a degenerate pose or flow that sends
// every source to one target is correct but serialised on that lane.
// ------------------------------------------------------------------------------------------------
// k_splat's skip rules for source pixel p of batch element b: returns the mask of in-frame corners (bit k: 0 = (x0,y0),
// 1 = (x0+1,y0), 2 = (x0,y0+1), 3 = (x0+1,y0+1)), the target of corner 0 and the four corner weights.
template <int MODE>
__device__ __forceinline__ int ord_corners(const float* __restrict__ flow, const float* __restrict__ valid, int b, int p, int H, int W,
                                           int& tnw, float w[4]) {
#pragma clang fp contract(off)
    const int HW = H * W, y = p / W, x = p - y * W;
    const float fx = (float)x + flow[((size_t)b * 2 + 0) * HW + p];
    const float fy = (float)y + flow[((size_t)b * 2 + 1) * HW + p];
    if (!isfinite(fx) || !isfinite(fy)) return 0;
    if (MODE == 1 && valid[(size_t)b * HW + p] == 0.f) return 0;
    const float x0f = floorf(fx), y0f = floorf(fy);
    if (!(x0f >= -2.f && x0f <= (float)W && y0f >= -2.f && y0f <= (float)H)) return 0;
    const int x0 = (int)x0f, y0 = (int)y0f;
    w[0] = ((float)(x0 + 1) - fx) * ((float)(y0 + 1) - fy);
    w[1] = (fx - (float)x0) * ((float)(y0 + 1) - fy);
    w[2] = ((float)(x0 + 1) - fx) * (fy - (float)y0);
    w[3] = (fx - (float)x0) * (fy - (float)y0);
    const bool xl = x0 >= 0 && x0 < W, xr = x0 + 1 >= 0 && x0 + 1 < W;
    const bool yt = y0 >= 0 && y0 < H, yb = y0 + 1 >= 0 && y0 + 1 < H;
    tnw = y0 * W + x0;
    return (xl && yt ? 1 : 0) | (xr && yt ? 2 : 0) | (xl && yb ? 4 : 0) | (xr && yb ? 8 : 0);
}

__device__ __forceinline__ int ord_target(int tnw, int k, int W) { return tnw + (k & 1) + (k >> 1) * W; }

// count[b*HW + t] += contributions to target t; MODE 1 also stores the source's exp(metric) scale (as k_splat computes it)
template <int MODE>
__global__ __launch_bounds__(256) void k_ord_count(const float* __restrict__ flow, const float* __restrict__ cur_disp,
                                                   const float* __restrict__ valid, const float* __restrict__ mean, int H, int W,
                                                   int* __restrict__ count, float* __restrict__ scale) {
    const int b = blockIdx.y, HW = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    int tnw;
    float w[4];
    const int m = ord_corners<MODE>(flow, valid, b, p, H, W, tnw, w);
    if (!m) return;
    if (MODE == 1) scale[(size_t)b * HW + p] = expf(fminf(fmaxf(cur_disp[(size_t)b * HW + p] - *mean, -50.f), 50.f));
    int* cb = count + (size_t)b * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (m & (1 << k)) atomicAdd(cb + ord_target(tnw, k, W), 1);
}

// exclusive prefix sum of one batch element's counts (one block per element): start = cursor = b*4*HW + offset, total[b] = entries
__global__ __launch_bounds__(1024) void k_ord_scan(const int* __restrict__ count, int HW, int* __restrict__ start, int* __restrict__ cursor,
                                                   int* __restrict__ total) {
    __shared__ int s[1024];
    const int b = blockIdx.x, t = threadIdx.x;
    const int per = (HW + 1023) / 1024, lo = min(HW, t * per), hi = min(HW, lo + per);
    const int* c = count + (size_t)b * HW;
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += c[i];
    s[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int run = b * 4 * HW + s[t] - sum;
    for (int i = lo; i < hi; ++i) {
        start[(size_t)b * HW + i] = run;
        cursor[(size_t)b * HW + i] = run;
        run += c[i];
    }
    if (t == 1023) total[b] = s[1023];
}

// every in-frame corner into its target's bucket, in arrival order: {source*4 + corner, weight bits, global target, 0}
template <int MODE>
__global__ __launch_bounds__(256) void k_ord_place(const float* __restrict__ flow, const float* __restrict__ valid, int H, int W,
                                                   int* __restrict__ cursor, int4* __restrict__ slots) {
    const int b = blockIdx.y, HW = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    int tnw;
    float w[4];
    const int m = ord_corners<MODE>(flow, valid, b, p, H, W, tnw, w);
    const int lim = (b + 1) * 4 * HW;            // the batch element's slot range (count and place apply the same rules)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!(m & (1 << k))) continue;
        const int gt = b * HW + ord_target(tnw, k, W);
        const int pos = atomicAdd(cursor + gt, 1);
        if (pos < lim) slots[pos] = make_int4(p * 4 + k, __float_as_int(w[k]), gt, 0);
    }
}

// entry -> sorted position: its bucket's start + the number of the bucket's entries with a smaller source index
__global__ __launch_bounds__(256) void k_ord_rank(const int4* __restrict__ slots, const int* __restrict__ start, const int* __restrict__ count,
                                                  const int* __restrict__ total, int HW, int2* __restrict__ sorted) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total[b]) return;
    const int4 e = slots[(size_t)b * 4 * HW + i];
    const int lo = start[e.z], n = count[e.z];
    int r = 0;
    for (int j = 0; j < n; ++j) r += slots[lo + j].x < e.x ? 1 : 0;
    sorted[lo + r] = make_int2(e.x >> 2, e.y);
}

// the first ORD_REG entries of a bucket are held in registers across the channel loop
#define ORD_REG 4

// one channel plane's sum over a sorted bucket: acc = (((0 + t_0) + t_1) + ...), t_j = (v[src_j] * s_j) * w_j (MODE 1) or v[src_j] * w_j
template <int MODE>
__device__ __forceinline__ float ord_plane_sum(const float* __restrict__ plane, const float* __restrict__ sc, const int2* __restrict__ list,
                                               int n, const int (&rs)[ORD_REG], const float (&rsc)[ORD_REG], const float (&rw)[ORD_REG]) {
#pragma clang fp contract(off)
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < ORD_REG; ++j)
        if (j < n) acc = acc + (MODE == 1 ? (plane[rs[j]] * rsc[j]) * rw[j] : plane[rs[j]] * rw[j]);
    for (int j = ORD_REG; j < n; ++j) {
        const int2 e = list[j];
        const float v = MODE == 1 ? plane[e.x] * sc[e.x] : plane[e.x];
        acc = acc + v * __int_as_float(e.y);
    }
    return acc;
}

template <int MODE>
__device__ __forceinline__ void ord_load_regs(const float* __restrict__ sc, const int2* __restrict__ list, int n, int (&rs)[ORD_REG],
                                              float (&rsc)[ORD_REG], float (&rw)[ORD_REG]) {
#pragma unroll
    for (int j = 0; j < ORD_REG; ++j) {
        const int2 e = j < n ? list[j] : make_int2(0, 0);
        rs[j] = e.x;
        rw[j] = __int_as_float(e.y);
        rsc[j] = (MODE == 1 && j < n) ? sc[e.x] : 0.f;
    }
}

// MODE 0: out[b, c, t] = ordered sum (tcs_softsplat_sum_ordered).  64 consecutive targets per block, channel quarters per wave.
__global__ __launch_bounds__(256) void k_ord_sum_gather(const int* __restrict__ start, const int* __restrict__ count,
                                                        const int2* __restrict__ sorted, const float* __restrict__ in, int C, int HW,
                                                        float* __restrict__ out) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + lane;
    if (p >= HW) return;
    const int lo = start[(size_t)b * HW + p], n = count[(size_t)b * HW + p];
    const int2* list = sorted + lo;
    int rs[ORD_REG];
    float rsc[ORD_REG], rw[ORD_REG];
    ord_load_regs<0>(nullptr, list, n, rs, rsc, rw);
    const int cq = (C + 3) / 4, c_lo = q * cq, c_hi = min(C, c_lo + cq);
    for (int c = c_lo; c < c_hi; ++c)
        out[((size_t)b * C + c) * HW + p] = ord_plane_sum<0>(in + ((size_t)b * C + c) * HW, nullptr, list, n, rs, rsc, rw);
}

// MODE 1: the ordered sums of warp() + k_warp_finish's normalisation, split and cosine cost, in k_warp_finish's layout and arithmetic.
// Channel order of the sums as k_splat's accumulator: [0,C) prev_fmap * s, C the new disparity * s, C+1 the normaliser s.
template <bool MIXED>
__device__ __forceinline__ void ord_warp_gather_body(const int* __restrict__ start, const int* __restrict__ count,
                                                     const int2* __restrict__ sorted, const float* __restrict__ prev_fmap,
                                                     const float* __restrict__ cur_disp, const float* __restrict__ scale,
                                                     const float* __restrict__ cur_fmap, const unsigned char* __restrict__ seq_start,
                                                     const float* __restrict__ prior_disp, const float* __restrict__ prior_cost,
                                                     const float* __restrict__ prior_mask, int C, int HW, float* __restrict__ out_disp,
                                                     float* __restrict__ out_fmap, float* __restrict__ out_mask, float* __restrict__ out_cost) {
#pragma clang fp contract(off)
    __shared__ float s_part[3][4][64];
    if (finish_start<MIXED>(seq_start, prior_disp, prior_cost, prior_mask, C, HW, out_disp, out_fmap, out_mask, out_cost)) return;
    const int b = blockIdx.y, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int p_raw = blockIdx.x * 64 + lane;
    const bool active = p_raw < HW;
    const int p = active ? p_raw : HW - 1;
    const int lo = start[(size_t)b * HW + p], n = count[(size_t)b * HW + p];
    const int2* list = sorted + lo;
    const float* sc = scale + (size_t)b * HW;
    int rs[ORD_REG];
    float rsc[ORD_REG], rw[ORD_REG];
    ord_load_regs<1>(sc, list, n, rs, rsc, rw);
    // normaliser (v = s) and disparity (v = cur_disp * s), summed in the same order as every other channel
    float norm = 0.f;
#pragma unroll
    for (int j = 0; j < ORD_REG; ++j)
        if (j < n) norm = norm + rsc[j] * rw[j];
    for (int j = ORD_REG; j < n; ++j) norm = norm + sc[list[j].x] * __int_as_float(list[j].y);
    const float mask = (norm != 0.f) ? 1.f : 0.f;
    const float den = fmaxf(norm, 1e-7f);
    if (q == 0 && active) {
        out_disp[(size_t)b * HW + p] = ord_plane_sum<1>(cur_disp + (size_t)b * HW, sc, list, n, rs, rsc, rw) / den;
        out_mask[(size_t)b * HW + p] = mask;
    }
    const int cq = (C + 3) / 4, c_lo = q * cq, c_hi = min(C, c_lo + cq);
    float dot = 0.f, n1 = 0.f, nw = 0.f;
    for (int c = c_lo; c < c_hi; ++c) {
        const float fw = ord_plane_sum<1>(prev_fmap + ((size_t)b * C + c) * HW, sc, list, n, rs, rsc, rw) / den;
        if (out_fmap && active) out_fmap[((size_t)b * C + c) * HW + p] = fw;
        if (out_cost) {
            const float f1 = cur_fmap[((size_t)b * C + c) * HW + p];
            dot = fmaf(f1, fw, dot);
            n1 = fmaf(f1, f1, n1);
            nw = fmaf(fw, fw, nw);
        }
    }
    if (!out_cost) return;
    s_part[0][q][lane] = dot; s_part[1][q][lane] = n1; s_part[2][q][lane] = nw;
    __syncthreads();
    if (q == 0 && active) {
        float t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = ((s_part[k][0][lane] + s_part[k][1][lane]) + s_part[k][2][lane]) + s_part[k][3][lane];
        out_cost[(size_t)b * HW + p] = t[0] / (fmaxf(sqrtf(t[1]), 1e-12f) * fmaxf(sqrtf(t[2]), 1e-12f)) * mask;
    }
}

__global__ __launch_bounds__(256) void k_ord_warp_gather(const int* __restrict__ start, const int* __restrict__ count,
                                                         const int2* __restrict__ sorted, const float* __restrict__ prev_fmap,
                                                         const float* __restrict__ cur_disp, const float* __restrict__ scale,
                                                         const float* __restrict__ cur_fmap, int C, int HW, float* __restrict__ out_disp,
                                                         float* __restrict__ out_fmap, float* __restrict__ out_mask, float* __restrict__ out_cost) {
    ord_warp_gather_body<false>(start, count, sorted, prev_fmap, cur_disp, scale, cur_fmap, nullptr, nullptr, nullptr, nullptr, C, HW,
                                out_disp, out_fmap, out_mask, out_cost);
}

__global__ __launch_bounds__(256) void k_ord_warp_gather_mixed(const int* __restrict__ start, const int* __restrict__ count,
                                                               const int2* __restrict__ sorted, const float* __restrict__ prev_fmap,
                                                               const float* __restrict__ cur_disp, const float* __restrict__ scale,
                                                               const float* __restrict__ cur_fmap, const unsigned char* __restrict__ seq_start,
                                                               const float* __restrict__ prior_disp, const float* __restrict__ prior_cost,
                                                               const float* __restrict__ prior_mask, int C, int HW,
                                                               float* __restrict__ out_disp, float* __restrict__ out_fmap,
                                                               float* __restrict__ out_mask, float* __restrict__ out_cost) {
    ord_warp_gather_body<true>(start, count, sorted, prev_fmap, cur_disp, scale, cur_fmap, seq_start, prior_disp, prior_cost, prior_mask,
                               C, HW, out_disp, out_fmap, out_mask, out_cost);
}

// ------------------------------------------------------------------------------------------------
// backward grid (geo_utils.py:201-236)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_backward_grid(const float* __restrict__ disp, const float* __restrict__ T_rel,
                                                       const float* __restrict__ K, const float* __restrict__ K_inv,
                                                       const float* __restrict__ baseline, int H, int W, float* __restrict__ grid) {
    const int b = blockIdx.y, HW = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const Cam c = load_cam(T_rel, K, K_inv, baseline, b);
    const int y = p / W, x = p - y * W;
    float zp, u, v;
    reproject(c, fmaxf(disp[(size_t)b * HW + p], 0.01f), (float)x, (float)y, zp, u, v);
    const bool ok = zp > 0.f;
    grid[((size_t)b * 2 + 0) * HW + p] = ok ? u : -1.f;
    grid[((size_t)b * 2 + 1) * HW + p] = ok ? v : -1.f;
}

// bilinear_sampler (utils.py:82-97): zeros padding, align_corners=True, pixel coordinates
// MIXED: a start element (start[b] != 0) gets +0.0 everywhere and reads neither img nor grid (the first frame's zero hidden states)
template <bool MIXED>
__device__ __forceinline__ void bilinear_sample_body(const float* __restrict__ img, const float* __restrict__ grid,
                                                     const unsigned char* __restrict__ start, int C, int Hi, int Wi, int HWo,
                                                     int ch_per_group, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HWo) return;
    if (MIXED && start[b]) {
        const int c_lo = blockIdx.z * ch_per_group, c_hi = min(C, c_lo + ch_per_group);
        for (int c = c_lo; c < c_hi; ++c) out[((size_t)b * C + c) * HWo + p] = 0.f;
        return;
    }
    float gx = grid[((size_t)b * 2 + 0) * HWo + p], gy = grid[((size_t)b * 2 + 1) * HWo + p];
    const bool fin = isfinite(gx) && isfinite(gy);
    gx = fminf(fmaxf(fin ? gx : -8.f, -8.f), (float)Wi + 8.f);
    gy = fminf(fmaxf(fin ? gy : -8.f, -8.f), (float)Hi + 8.f);
    const float x0f = floorf(gx), y0f = floorf(gy);
    const float ax = gx - x0f, ay = gy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const bool xl = x0 >= 0 && x0 < Wi, xr = x0 + 1 >= 0 && x0 + 1 < Wi;
    const bool yt = y0 >= 0 && y0 < Hi, yb = y0 + 1 >= 0 && y0 + 1 < Hi;
    const int o00 = y0 * Wi + x0;
    const int c_lo = blockIdx.z * ch_per_group, c_hi = min(C, c_lo + ch_per_group);
    const size_t HWi = (size_t)Hi * Wi;
    for (int c = c_lo; c < c_hi; ++c) {
        const float* s = img + ((size_t)b * C + c) * HWi + o00;
        const float v00 = (xl && yt) ? s[0] : 0.f;
        const float v01 = (xr && yt) ? s[1] : 0.f;
        const float v10 = (xl && yb) ? s[Wi] : 0.f;
        const float v11 = (xr && yb) ? s[Wi + 1] : 0.f;
        const float top = (1.f - ax) * v00 + ax * v01;
        const float bot = (1.f - ax) * v10 + ax * v11;
        out[((size_t)b * C + c) * HWo + p] = (1.f - ay) * top + ay * bot;
    }
}

__global__ __launch_bounds__(256) void k_bilinear_sample(const float* __restrict__ img, const float* __restrict__ grid,
                                                         int C, int Hi, int Wi, int HWo, int ch_per_group,
                                                         float* __restrict__ out) {
    bilinear_sample_body<false>(img, grid, nullptr, C, Hi, Wi, HWo, ch_per_group, out);
}

__global__ __launch_bounds__(256) void k_bilinear_sample_mixed(const float* __restrict__ img, const float* __restrict__ grid,
                                                               const unsigned char* __restrict__ start, int C, int Hi, int Wi, int HWo,
                                                               int ch_per_group, float* __restrict__ out) {
    bilinear_sample_body<true>(img, grid, start, C, Hi, Wi, HWo, ch_per_group, out);
}

// bilinear resize, align_corners=True (F.interpolate), times `scale`
__global__ __launch_bounds__(256) void k_resize_bilinear(const float* __restrict__ x, int C, int H, int W, int Ho, int Wo,
                                                         float scale, float* __restrict__ out) {
    const int bc = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Ho * Wo) return;
    const int yo = p / Wo, xo = p - yo * Wo;
    const float sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f;
    const float sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    const float fy = sy * (float)yo, fx = sx * (float)xo;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < H - 1), x1 = x0 + (x0 < W - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float* s = x + (size_t)bc * H * W;
    const float v = (1.f - ly) * ((1.f - lx) * s[y0 * W + x0] + lx * s[y0 * W + x1]) +
                    ly * ((1.f - lx) * s[y1 * W + x0] + lx * s[y1 * W + x1]);
    out[(size_t)bc * Ho * Wo + p] = scale * v;
}

// ------------------------------------------------------------------------------------------------
// camera algebra of tc_stereo.py:121-127,159 on the device (one thread per batch element): keeps the
// frame free of host round trips (torch.linalg.inv synchronises) so it can be captured in a HIP graph.
// ------------------------------------------------------------------------------------------------
template <int N>
__device__ void invert_small(const float* __restrict__ m, float* __restrict__ inv) {
    float a[N][2 * N];
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) { a[i][j] = m[i * N + j]; a[i][N + j] = (i == j) ? 1.f : 0.f; }
    for (int c = 0; c < N; ++c) {                      // Gauss-Jordan, partial pivoting
        int p = c;
        for (int r = c + 1; r < N; ++r) if (fabsf(a[r][c]) > fabsf(a[p][c])) p = r;
        if (p != c) for (int j = 0; j < 2 * N; ++j) { const float t = a[c][j]; a[c][j] = a[p][j]; a[p][j] = t; }
        const float piv = 1.0f / a[c][c];
        for (int j = 0; j < 2 * N; ++j) a[c][j] *= piv;
        for (int r = 0; r < N; ++r) {
            if (r == c) continue;
            const float f = a[r][c];
            for (int j = 0; j < 2 * N; ++j) a[r][j] = fmaf(-f, a[c][j], a[r][j]);
        }
    }
    for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) inv[i * N + j] = a[i][N + j];
}

__device__ void matmul4(const float* a, const float* b, float* o) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
            for (int k = 0; k < 4; ++k) s = fmaf(a[i * 4 + k], b[k * 4 + j], s);
            o[i * 4 + j] = s;
        }
}

// MIXED: a start element (start[b] != 0) gets identity T_rel / T_back without reading its T or T_prev; its K is scaled as usual
template <bool MIXED>
__device__ __forceinline__ void pose_prepare_body(const float* __restrict__ K, const float* __restrict__ T, const float* __restrict__ Tp,
                                                  const unsigned char* __restrict__ start, float scale, int B, float* __restrict__ Ks,
                                                  float* __restrict__ Ksi, float* __restrict__ Trel, float* __restrict__ Tback) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float ks[9], inv3[9];
    for (int i = 0; i < 9; ++i) ks[i] = K[b * 9 + i] * (i < 6 ? scale : 1.f);     // rows 0,1 scaled (tc_stereo.py:122)
    invert_small<3>(ks, inv3);
    for (int i = 0; i < 9; ++i) { Ks[b * 9 + i] = ks[i]; Ksi[b * 9 + i] = inv3[i]; }
    if (MIXED && start[b]) {
        for (int i = 0; i < 16; ++i) Trel[b * 16 + i] = Tback[b * 16 + i] = (i % 5 == 0) ? 1.f : 0.f;
        return;
    }
    if (T && Tp) {
        float inv4[16], o[16];
        invert_small<4>(Tp + b * 16, inv4);
        matmul4(T + b * 16, inv4, o);                                             // geo_utils.py:148-155
        for (int i = 0; i < 16; ++i) Trel[b * 16 + i] = o[i];
        invert_small<4>(T + b * 16, inv4);
        matmul4(Tp + b * 16, inv4, o);                                            // tc_stereo.py:159
        for (int i = 0; i < 16; ++i) Tback[b * 16 + i] = o[i];
    }
}

__global__ void k_pose_prepare(const float* __restrict__ K, const float* __restrict__ T, const float* __restrict__ Tp, float scale,
                               int B, float* __restrict__ Ks, float* __restrict__ Ksi, float* __restrict__ Trel,
                               float* __restrict__ Tback) {
    pose_prepare_body<false>(K, T, Tp, nullptr, scale, B, Ks, Ksi, Trel, Tback);
}

__global__ void k_pose_prepare_mixed(const float* __restrict__ K, const float* __restrict__ T, const float* __restrict__ Tp,
                                     const unsigned char* __restrict__ start, float scale, int B, float* __restrict__ Ks,
                                     float* __restrict__ Ksi, float* __restrict__ Trel, float* __restrict__ Tback) {
    pose_prepare_body<true>(K, T, Tp, start, scale, B, Ks, Ksi, Trel, Tback);
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct WarpWs {
    float *cur_disp, *valid, *flow, *partial, *mean, *acc;
    size_t acc_bytes;
};

static WarpWs carve(void* ws, int B, int C, int H, int W) {
    const size_t HW = (size_t)H * W;
    char* p = reinterpret_cast<char*>(ws);
    WarpWs w;
    w.cur_disp = reinterpret_cast<float*>(p); p += al256(B * HW * 4);
    w.valid = reinterpret_cast<float*>(p);    p += al256(B * HW * 4);
    w.flow = reinterpret_cast<float*>(p);     p += al256(2 * B * HW * 4);
    w.partial = reinterpret_cast<float*>(p);  p += al256((size_t)B * tcs_cdiv(HW, 256) * 4);
    w.mean = reinterpret_cast<float*>(p);     p += 256;
    w.acc = reinterpret_cast<float*>(p);
    w.acc_bytes = (size_t)B * (C + 2) * HW * 4;
    return w;
}

// the inverted index of the ordered splat; `scale` only for warp()
struct OrdWs {
    int *count, *start, *cursor, *total;
    int4* slots;
    int2* sorted;
    float* scale;
    size_t count_bytes;
};

static size_t ord_bytes(int B, size_t HW, bool with_scale) {
    const size_t n = (size_t)B * HW;
    return al256(n * 4) * 3 + al256((size_t)B * 4) + al256(4 * n * sizeof(int4)) + al256(4 * n * sizeof(int2)) + (with_scale ? al256(n * 4) : 0);
}

static OrdWs carve_ord(void* ws, int B, size_t HW, bool with_scale) {
    const size_t n = (size_t)B * HW;
    char* p = reinterpret_cast<char*>(ws);
    OrdWs o;
    o.count = reinterpret_cast<int*>(p);    o.count_bytes = al256(n * 4); p += o.count_bytes;
    o.start = reinterpret_cast<int*>(p);    p += al256(n * 4);
    o.cursor = reinterpret_cast<int*>(p);   p += al256(n * 4);
    o.total = reinterpret_cast<int*>(p);    p += al256((size_t)B * 4);
    o.slots = reinterpret_cast<int4*>(p);   p += al256(4 * n * sizeof(int4));
    o.sorted = reinterpret_cast<int2*>(p);  p += al256(4 * n * sizeof(int2));
    o.scale = with_scale ? reinterpret_cast<float*>(p) : nullptr;
    return o;
}

// the B*4*HW slot positions and source*4 + corner keys are ints; the scan runs one block per batch element
static bool ord_dims_ok(int B, int H, int W) { return (long long)B * 4 * H * W <= 0x7fffffffLL && B <= 65535; }

// count -> scan -> place -> rank for a splat along `flow`; MODE 1 also fills o.scale
template <int MODE>
static void ord_index(const float* flow, const float* cur_disp, const float* valid, const float* mean, int B, int H, int W, const OrdWs& o,
                      hipStream_t s) {
    const int HW = H * W, nb = tcs_cdiv(HW, 256);
    const size_t n4 = o.count_bytes / 16;
    hipLaunchKernelGGL(k_zero_fill, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<float4*>(o.count), n4);
    hipLaunchKernelGGL(k_ord_count<MODE>, dim3(nb, B), dim3(256), 0, s, flow, cur_disp, valid, mean, H, W, o.count, o.scale);
    hipLaunchKernelGGL(k_ord_scan, dim3(B), dim3(1024), 0, s, o.count, HW, o.start, o.cursor, o.total);
    hipLaunchKernelGGL(k_ord_place<MODE>, dim3(nb, B), dim3(256), 0, s, flow, valid, H, W, o.cursor, o.slots);
    hipLaunchKernelGGL(k_ord_rank, dim3(tcs_cdiv(4LL * HW, 256), B), dim3(256), 0, s, o.slots, o.start, o.count, o.total, HW, o.sorted);
}

extern "C" {

size_t tcs_warp_ordered_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C < 0 || H <= 0 || W <= 0) return 0;
    const size_t HW = (size_t)H * W;
    return al256(B * HW * 4) * 2 + al256(2 * B * HW * 4) + al256((size_t)B * tcs_cdiv(HW, 256) * 4) + 256 + ord_bytes(B, HW, true);
}

size_t tcs_softsplat_ordered_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return ord_bytes(B, (size_t)H * W, false);
}

size_t tcs_warp_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C < 0 || H <= 0 || W <= 0) return 0;
    const size_t HW = (size_t)H * W;
    return al256(B * HW * 4) * 2 + al256(2 * B * HW * 4) + al256((size_t)B * tcs_cdiv(HW, 256) * 4) + 256 +
           al256((size_t)B * (C + 2) * HW * 4);
}

// `start` (device, [B]): the mixed geometry (start elements skipped, the mean over the temporal elements' pixels); nullptr: today's
static int geometry(const float* prev_disp, const float* T_rel, const float* K, const float* K_inv, const float* baseline,
                    int B, int H, int W, const WarpWs& w, hipStream_t s, const unsigned char* start = nullptr) {
    const int nb = tcs_cdiv((long long)H * W, 256);
    if (start) {
        hipLaunchKernelGGL(k_warp_geometry_mixed, dim3(nb, B), dim3(256), 0, s, prev_disp, T_rel, K, K_inv, baseline, start, H, W,
                           w.cur_disp, w.valid, w.flow, w.partial);
        hipLaunchKernelGGL(k_mean_mixed, dim3(1), dim3(256), 0, s, w.partial, nb * B, start, B, (long long)H * W, w.mean);
        return tcs_launch_status();
    }
    hipLaunchKernelGGL(k_warp_geometry, dim3(nb, B), dim3(256), 0, s, prev_disp, T_rel, K, K_inv, baseline, H, W,
                       w.cur_disp, w.valid, w.flow, w.partial);
    hipLaunchKernelGGL(k_mean, dim3(1), dim3(256), 0, s, w.partial, nb * B, 1.0f / (float)((long long)B * H * W), w.mean);
    return tcs_launch_status();
}

int tcs_warp_geometry(const float* prev_disp, const float* T_rel, const float* K, const float* K_inv,
                      const float* baseline, int B, int H, int W,
                      float* cur_disp, float* valid, float* flow, float* metric, void* workspace, tcs_stream_t stream) {
    if (!prev_disp || !T_rel || !K || !K_inv || !baseline || !cur_disp || !valid || !flow || !metric || !workspace)
        return TCS_EINVAL;
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0) return TCS_EINVAL;
    hipStream_t s = tcs_stream(stream);
    WarpWs w = carve(workspace, B, 0, H, W);
    w.cur_disp = cur_disp; w.valid = valid; w.flow = flow;
    int rc = geometry(prev_disp, T_rel, K, K_inv, baseline, B, H, W, w, s);
    if (rc) return rc;
    const int n = B * H * W;
    hipLaunchKernelGGL(k_metric, dim3(tcs_cdiv(n, 256)), dim3(256), 0, s, cur_disp, w.mean, n, metric);
    return tcs_launch_status();
}

int tcs_warp_forward(const float* prev_disp, const float* prev_fmap, const float* T_rel, const float* K,
                     const float* K_inv, const float* baseline, int B, int C, int H, int W,
                     float* out_disp, float* out_fmap, float* out_mask, const float* cur_fmap, float* out_cost,
                     void* workspace, tcs_stream_t stream) {
    if (!prev_disp || !prev_fmap || !T_rel || !K || !K_inv || !baseline || !out_disp || !out_mask || !workspace)
        return TCS_EINVAL;
    if ((cur_fmap == nullptr) != (out_cost == nullptr)) return TCS_EINVAL;
    if (B <= 0 || B > 65535 || C <= 0 || H <= 0 || W <= 0) return TCS_EINVAL;
    hipStream_t s = tcs_stream(stream);
    WarpWs w = carve(workspace, B, C, H, W);
    int rc = geometry(prev_disp, T_rel, K, K_inv, baseline, B, H, W, w, s);
    if (rc) return rc;
    {
        const size_t n4 = (w.acc_bytes + 15) / 16;          // the carve is 256-byte aligned and padded
        hipLaunchKernelGGL(k_zero_fill, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<float4*>(w.acc), n4);
    }
    const int nb = tcs_cdiv((long long)H * W, 256);
    const int cpg = 16, groups = tcs_cdiv(C + 2, cpg);
    hipLaunchKernelGGL(k_splat<1>, dim3(nb, B, groups), dim3(256), 0, s, prev_fmap, w.flow, w.cur_disp, w.valid, w.mean,
                       C, H, W, cpg, w.acc);
    hipLaunchKernelGGL(k_warp_finish, dim3(tcs_cdiv((long long)H * W, 64), B), dim3(256), 0, s, w.acc, cur_fmap, C, H * W, out_disp, out_fmap,
                       out_mask, out_cost);
    return tcs_launch_status();
}

int tcs_warp_forward_mixed(const float* prev_disp, const float* prev_fmap, const float* T_rel, const float* K,
                           const float* K_inv, const float* baseline, const unsigned char* start, const float* prior_disp,
                           const float* prior_cost, const float* prior_mask, int B, int C, int H, int W,
                           float* out_disp, float* out_fmap, float* out_mask, const float* cur_fmap, float* out_cost,
                           void* workspace, tcs_stream_t stream) {
    if (!prev_disp || !prev_fmap || !T_rel || !K || !K_inv || !baseline || !out_disp || !out_mask || !workspace)
        return TCS_EINVAL;
    if (!start || !prior_disp || !prior_cost || !prior_mask) return TCS_EINVAL;
    if ((cur_fmap == nullptr) != (out_cost == nullptr)) return TCS_EINVAL;
    if (B <= 0 || B > 65535 || C <= 0 || H <= 0 || W <= 0) return TCS_EINVAL;
    hipStream_t s = tcs_stream(stream);
    WarpWs w = carve(workspace, B, C, H, W);
    int rc = geometry(prev_disp, T_rel, K, K_inv, baseline, B, H, W, w, s, start);
    if (rc) return rc;
    {
        const size_t n4 = (w.acc_bytes + 15) / 16;
        hipLaunchKernelGGL(k_zero_fill, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<float4*>(w.acc), n4);
    }
    const int nb = tcs_cdiv((long long)H * W, 256);
    const int cpg = 16, groups = tcs_cdiv(C + 2, cpg);
    // (start elements have valid = 0 everywhere: k_splat skips every one of their pixels)
    hipLaunchKernelGGL(k_splat<1>, dim3(nb, B, groups), dim3(256), 0, s, prev_fmap, w.flow, w.cur_disp, w.valid, w.mean,
                       C, H, W, cpg, w.acc);
    hipLaunchKernelGGL(k_warp_finish_mixed, dim3(tcs_cdiv((long long)H * W, 64), B), dim3(256), 0, s, w.acc, cur_fmap, start, prior_disp,
                       prior_cost, prior_mask, C, H * W, out_disp, out_fmap, out_mask, out_cost);
    return tcs_launch_status();
}

int tcs_softsplat_sum(const float* in, const float* flow, int B, int C, int H, int W, float* out, tcs_stream_t stream) {
    if (!in || !flow || !out || B <= 0 || B > 65535 || C <= 0 || H <= 0 || W <= 0) return TCS_EINVAL;
    const int nb = tcs_cdiv((long long)H * W, 256);
    const int cpg = 16, groups = tcs_cdiv(C, cpg);
    hipLaunchKernelGGL(k_splat<0>, dim3(nb, B, groups), dim3(256), 0, tcs_stream(stream), in, flow,
                       (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, C, H, W, cpg, out);
    return tcs_launch_status();
}

int tcs_warp_forward_ordered(const float* prev_disp, const float* prev_fmap, const float* T_rel, const float* K,
                             const float* K_inv, const float* baseline, int B, int C, int H, int W,
                             float* out_disp, float* out_fmap, float* out_mask, const float* cur_fmap, float* out_cost,
                             void* workspace, tcs_stream_t stream) {
    if (!prev_disp || !prev_fmap || !T_rel || !K || !K_inv || !baseline || !out_disp || !out_mask || !workspace)
        return TCS_EINVAL;
    if ((cur_fmap == nullptr) != (out_cost == nullptr)) return TCS_EINVAL;
    if (B <= 0 || B > 65535 || C <= 0 || H <= 0 || W <= 0 || !ord_dims_ok(B, H, W)) return TCS_EINVAL;
    hipStream_t s = tcs_stream(stream);
    const WarpWs w = carve(workspace, B, C, H, W);
    int rc = geometry(prev_disp, T_rel, K, K_inv, baseline, B, H, W, w, s);
    if (rc) return rc;
    const OrdWs o = carve_ord(w.acc, B, (size_t)H * W, true);          // the ordered index sits where the atomic path's accumulator does
    ord_index<1>(w.flow, w.cur_disp, w.valid, w.mean, B, H, W, o, s);
    hipLaunchKernelGGL(k_ord_warp_gather, dim3(tcs_cdiv((long long)H * W, 64), B), dim3(256), 0, s, o.start, o.count, o.sorted, prev_fmap,
                       w.cur_disp, o.scale, cur_fmap, C, H * W, out_disp, out_fmap, out_mask, out_cost);
    return tcs_launch_status();
}

int tcs_warp_forward_ordered_mixed(const float* prev_disp, const float* prev_fmap, const float* T_rel, const float* K,
                                   const float* K_inv, const float* baseline, const unsigned char* start, const float* prior_disp,
                                   const float* prior_cost, const float* prior_mask, int B, int C, int H, int W,
                                   float* out_disp, float* out_fmap, float* out_mask, const float* cur_fmap, float* out_cost,
                                   void* workspace, tcs_stream_t stream) {
    if (!prev_disp || !prev_fmap || !T_rel || !K || !K_inv || !baseline || !out_disp || !out_mask || !workspace)
        return TCS_EINVAL;
    if (!start || !prior_disp || !prior_cost || !prior_mask) return TCS_EINVAL;
    if ((cur_fmap == nullptr) != (out_cost == nullptr)) return TCS_EINVAL;
    if (B <= 0 || B > 65535 || C <= 0 || H <= 0 || W <= 0 || !ord_dims_ok(B, H, W)) return TCS_EINVAL;
    hipStream_t s = tcs_stream(stream);
    const WarpWs w = carve(workspace, B, C, H, W);
    int rc = geometry(prev_disp, T_rel, K, K_inv, baseline, B, H, W, w, s, start);
    if (rc) return rc;
    const OrdWs o = carve_ord(w.acc, B, (size_t)H * W, true);
    ord_index<1>(w.flow, w.cur_disp, w.valid, w.mean, B, H, W, o, s);         // (valid = 0: no index entries for start elements)
    hipLaunchKernelGGL(k_ord_warp_gather_mixed, dim3(tcs_cdiv((long long)H * W, 64), B), dim3(256), 0, s, o.start, o.count, o.sorted,
                       prev_fmap, w.cur_disp, o.scale, cur_fmap, start, prior_disp, prior_cost, prior_mask, C, H * W, out_disp, out_fmap,
                       out_mask, out_cost);
    return tcs_launch_status();
}

int tcs_softsplat_sum_ordered(const float* in, const float* flow, int B, int C, int H, int W, float* out, void* workspace,
                              tcs_stream_t stream) {
    if (!in || !flow || !out || !workspace || B <= 0 || B > 65535 || C <= 0 || H <= 0 || W <= 0 || !ord_dims_ok(B, H, W))
        return TCS_EINVAL;
    hipStream_t s = tcs_stream(stream);
    const OrdWs o = carve_ord(workspace, B, (size_t)H * W, false);
    ord_index<0>(flow, nullptr, nullptr, nullptr, B, H, W, o, s);
    hipLaunchKernelGGL(k_ord_sum_gather, dim3(tcs_cdiv((long long)H * W, 64), B), dim3(256), 0, s, o.start, o.count, o.sorted, in, C, H * W,
                       out);
    return tcs_launch_status();
}

int tcs_backward_grid(const float* disp, const float* T_rel, const float* K, const float* K_inv,
                      const float* baseline, int B, int H, int W, float* grid, tcs_stream_t stream) {
    if (!disp || !T_rel || !K || !K_inv || !baseline || !grid || B <= 0 || B > 65535 || H <= 0 || W <= 0) return TCS_EINVAL;
    hipLaunchKernelGGL(k_backward_grid, dim3(tcs_cdiv((long long)H * W, 256), B), dim3(256), 0, tcs_stream(stream),
                       disp, T_rel, K, K_inv, baseline, H, W, grid);
    return tcs_launch_status();
}

int tcs_bilinear_sample(const float* img, const float* grid, int B, int C, int Hi, int Wi, int Ho, int Wo,
                        float* out, tcs_stream_t stream) {
    if (!img || !grid || !out || B <= 0 || B > 65535 || C <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0) return TCS_EINVAL;
    const int cpg = 16;
    hipLaunchKernelGGL(k_bilinear_sample, dim3(tcs_cdiv((long long)Ho * Wo, 256), B, tcs_cdiv(C, cpg)), dim3(256), 0,
                       tcs_stream(stream), img, grid, C, Hi, Wi, Ho * Wo, cpg, out);
    return tcs_launch_status();
}

int tcs_bilinear_sample_mixed(const float* img, const float* grid, const unsigned char* start, int B, int C, int Hi, int Wi, int Ho,
                              int Wo, float* out, tcs_stream_t stream) {
    if (!img || !grid || !start || !out || B <= 0 || B > 65535 || C <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0) return TCS_EINVAL;
    const int cpg = 16;
    hipLaunchKernelGGL(k_bilinear_sample_mixed, dim3(tcs_cdiv((long long)Ho * Wo, 256), B, tcs_cdiv(C, cpg)), dim3(256), 0,
                       tcs_stream(stream), img, grid, start, C, Hi, Wi, Ho * Wo, cpg, out);
    return tcs_launch_status();
}

int tcs_grid_halve(const float* grid, int B, int H, int W, float* out, tcs_stream_t stream) {
    if (!grid || !out || B <= 0 || H < 2 || W < 2) return TCS_EINVAL;
    const int Ho = H / 2, Wo = W / 2;
    hipLaunchKernelGGL(k_resize_bilinear, dim3(tcs_cdiv((long long)Ho * Wo, 256), B * 2), dim3(256), 0, tcs_stream(stream),
                       grid, 2, H, W, Ho, Wo, 0.5f, out);
    return tcs_launch_status();
}

int tcs_pose_prepare(const float* K, const float* T, const float* T_prev, float scale, int B,
                     float* K_scaled, float* K_scaled_inv, float* T_rel, float* T_back, tcs_stream_t stream) {
    if (!K || !K_scaled || !K_scaled_inv || B <= 0) return TCS_EINVAL;
    if ((T == nullptr) != (T_prev == nullptr)) return TCS_EINVAL;
    if (T && (!T_rel || !T_back)) return TCS_EINVAL;
    hipLaunchKernelGGL(k_pose_prepare, dim3(tcs_cdiv(B, 64)), dim3(64), 0, tcs_stream(stream), K, T, T_prev, scale, B,
                       K_scaled, K_scaled_inv, T_rel, T_back);
    return tcs_launch_status();
}

int tcs_pose_prepare_mixed(const float* K, const float* T, const float* T_prev, const unsigned char* start, float scale, int B,
                           float* K_scaled, float* K_scaled_inv, float* T_rel, float* T_back, tcs_stream_t stream) {
    if (!K || !T || !T_prev || !start || !K_scaled || !K_scaled_inv || !T_rel || !T_back || B <= 0) return TCS_EINVAL;
    hipLaunchKernelGGL(k_pose_prepare_mixed, dim3(tcs_cdiv(B, 64)), dim3(64), 0, tcs_stream(stream), K, T, T_prev, start, scale, B,
                       K_scaled, K_scaled_inv, T_rel, T_back);
    return tcs_launch_status();
}

int tcs_resize_bilinear(const float* x, int B, int C, int H, int W, int Ho, int Wo, float* out, tcs_stream_t stream) {
    if (!x || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return TCS_EINVAL;
    if ((long long)B * C > 65535) return TCS_EUNSUPPORTED;
    hipLaunchKernelGGL(k_resize_bilinear, dim3(tcs_cdiv((long long)Ho * Wo, 256), B * C), dim3(256), 0, tcs_stream(stream),
                       x, C, H, W, Ho, Wo, 1.0f, out);
    return tcs_launch_status();
}

int tcs_resize_bilinear_scaled(const float* x, int B, int C, int H, int W, int Ho, int Wo, float scale, float* out, tcs_stream_t stream) {
    if (!x || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return TCS_EINVAL;
    if ((long long)B * C > 65535) return TCS_EUNSUPPORTED;
    hipLaunchKernelGGL(k_resize_bilinear, dim3(tcs_cdiv((long long)Ho * Wo, 256), B * C), dim3(256), 0, tcs_stream(stream),
                       x, C, H, W, Ho, Wo, scale, out);
    return tcs_launch_status();
}

}  // extern "C"
