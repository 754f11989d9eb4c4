// The reference's training objective (train_stereo.py:41-160, 362-399) on gfx950: the quarter-resolution targets, sequence_loss,
// init_loss, disp_grad_loss and disp_normal_loss, and one finishing launch that turns the per-block partial sums into the losses and
// the metrics.  Per-element arithmetic is fp32 in the reference's operation order; every sum is fp64, written per block and finished in
// a fixed order (no float atomics), so two calls are bit-equal.  A non-finite prediction is counted in a partial slot and reported in
// the output vector, in place of the reference's asserts.
#include "tcs_common.h"

// The masks compare rounded fp32 values (`== 1` after bilinear interpolation, `/` before `< 5`, the +-1.5 window), so nothing in this
// file may be contracted to an FMA: each operation rounds where PyTorch's separate ops round.  The one FMA below is written out.
#pragma clang fp contract(off)

#define LOSS_NT 256          // threads per block of every partial-sum kernel
#define SEQ_PIX 4            // full-resolution pixels per thread of the sequence kernel
#define LOSS_MAX_K 8

namespace {

// Correctly rounded fp32 quotient and square root, as the CPU computes them: formed in fp64 and rounded once (exact for fp32
// operands: fp64 carries more than 2 * 24 + 2 bits).  The fp32 device sequences are not correctly rounded on every build.
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float sqrt_rn(float a) { return (float)__dsqrt_rn((double)a); }

// valid_mode: 0 = float values as given (the caller's valid.float()), 1 = the trainer's rule on the dataset's raw valid,
// (valid >= 0.5) & (|flow| < 700) (train_stereo.py:366-369), 2 = a bool / uint8 mask
__device__ __forceinline__ float valid_at(const void* v, int mode, const float* flow, long long p) {
    if (mode == 2) return reinterpret_cast<const uint8_t*>(v)[p] ? 1.f : 0.f;
    const float x = reinterpret_cast<const float*>(v)[p];
    if (mode == 0) return x;
    const float f = flow[p];
    return (x >= 0.5f && sqrt_rn(__fmul_rn(f, f)) < 700.f) ? 1.f : 0.f;
}

// F.interpolate(valid, scale_factor=1/4, mode='bilinear', align_corners=True) == 1 at quarter pixel (y, x) of one image: PyTorch CPU's
// index rule (scale (in-1)/(out-1) in fp32, index floor clamped, lambda clamped to [0,1]) and the operation order of its channels-last
// kernel, which is the one a 1-channel [B,1,H,W] map takes (it is channels-last contiguous too):
// ((h0l*w0l) * v00 + (h0l*w1l) * v01) + (h1l*w0l) * v10) + (h1l*w1l) * v11
__device__ __forceinline__ bool bilinear_is_one(const void* v, int mode, const float* flow, long long img, int H, int W, int h, int w,
                                                int y, int x) {
    const float sh = h > 1 ? div_rn((float)(H - 1), (float)(h - 1)) : 0.f;
    const float sw = w > 1 ? div_rn((float)(W - 1), (float)(w - 1)) : 0.f;
    const float ry = sh * (float)y, rx = sw * (float)x;
    const int y0 = min((int)floorf(ry), H - 1), x0 = min((int)floorf(rx), W - 1);
    const float h1l = fminf(fmaxf(ry - (float)y0, 0.f), 1.f), w1l = fminf(fmaxf(rx - (float)x0, 0.f), 1.f);
    const float h0l = 1.f - h1l, w0l = 1.f - w1l;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float v00 = valid_at(v, mode, flow, img + (long long)y0 * W + x0), v01 = valid_at(v, mode, flow, img + (long long)y0 * W + x1);
    const float v10 = valid_at(v, mode, flow, img + (long long)y1 * W + x0), v11 = valid_at(v, mode, flow, img + (long long)y1 * W + x1);
    return ((((h0l * w0l) * v00 + (h0l * w1l) * v01) + (h1l * w0l) * v10) + (h1l * w1l) * v11) == 1.f;
}

// F.max_pool2d(valid, 4, 4, 0).bool() at quarter pixel (y, x)
__device__ __forceinline__ bool maxpool_nonzero(const void* v, int mode, const float* flow, long long img, int W, int y, int x) {
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) m = fmaxf(m, valid_at(v, mode, flow, img + (long long)(4 * y + i) * W + 4 * x + j));
    return m != 0.f;
}

// torch.median over 16 values (the lower median, sorted index 7; NaN if any is NaN): a bitonic sorting network in registers
__device__ __forceinline__ float median16(float (&a)[16]) {
    bool nan = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) nan |= isnan(a[i]);
#pragma unroll
    for (int k = 2; k <= 16; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const float lo = fminf(a[i], a[l]), hi = fmaxf(a[i], a[l]);
                    const bool up = (i & k) == 0;
                    a[i] = up ? lo : hi;
                    a[l] = up ? hi : lo;
                }
            }
    return nan ? NAN : a[7];
}

// F.normalize((gx, gy, -1), dim=1) as PyTorch CPU computes it: the vectorised 2-norm fuses the squares,
// sqrt(fma(-1, -1, fma(gy, gy, gx * gx))), and the quotient uses norm.clamp_min(1e-12)
__device__ __forceinline__ float normal_rnorm_denominator(float gx, float gy) {
    const float s = __fadd_rn(__fmaf_rn(gy, gy, __fmul_rn(gx, gx)), 1.f);
    return fmaxf(sqrt_rn(s), 1e-12f);
}

// fixed-order block sum of M doubles; the result is valid on thread 0
template <int M>
__device__ __forceinline__ void block_sum(double (&v)[M], double (*sh)[LOSS_NT / TCS_WAVE]) {
    const int lane = threadIdx.x & (TCS_WAVE - 1), wid = threadIdx.x / TCS_WAVE;
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[m] += __shfl_down(v[m], o, TCS_WAVE);
    __syncthreads();                                    // the previous call's readers are done with sh
    if (lane == 0)
#pragma unroll
        for (int m = 0; m < M; ++m) sh[m][wid] = v[m];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int m = 0; m < M; ++m) {
            double t = 0.0;
#pragma unroll
            for (int i = 0; i < LOSS_NT / TCS_WAVE; ++i) t += sh[m][i];
            v[m] = t;
        }
}

__device__ __forceinline__ bool finite(float x) { return isfinite(x); }

// ---------------------------------------------------------------------------------------------------------------------------------
// quarter-resolution targets
// ---------------------------------------------------------------------------------------------------------------------------------
// From the flow: per quarter pixel the 4x4 window of the replicate-padded forward differences of -flow (geo_utils.py:115-132), their
// normals, the lower median of each channel, the GT masks, and the dense / sparse valid masks.  The full-resolution maps never exist.
__global__ __launch_bounds__(LOSS_NT) void k_loss_targets(const float* __restrict__ flow, const void* __restrict__ valid, int vmode,
                                                          int B, int H, int W, float* __restrict__ grad_gt, float* __restrict__ norm_gt,
                                                          uint8_t* __restrict__ grad_mask, uint8_t* __restrict__ norm_mask,
                                                          uint8_t* __restrict__ valid_dense, uint8_t* __restrict__ valid_sparse) {
    const int h = H / 4, w = W / 4;
    const long long n = (long long)B * h * w;
    const long long p = (long long)blockIdx.x * LOSS_NT + threadIdx.x;
    if (p >= n) return;
    const int x = (int)(p % w), y = (int)((p / w) % h), b = (int)(p / ((long long)h * w));
    const long long img = (long long)b * H * W;
    float d[5][5];                                      // -flow on rows 4y..4y+4, columns 4x..4x+4, replicate-clamped
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) d[i][j] = -flow[img + (long long)min(4 * y + i, H - 1) * W + min(4 * x + j, W - 1)];
    float gx[16], gy[16], a[16];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            gx[4 * i + j] = d[i][j + 1] - d[i][j];
            gy[4 * i + j] = d[i + 1][j] - d[i][j];
        }
    const long long hw = (long long)h * w, q = (long long)y * w + x;
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = gx[i];
    const float mgx = median16(a);
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = gy[i];
    const float mgy = median16(a);
    grad_gt[(long long)b * 2 * hw + q] = mgx;
    grad_gt[((long long)b * 2 + 1) * hw + q] = mgy;
    grad_mask[p] = mgx < 5.f && mgy < 5.f;
    float nrm[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) nrm[i] = normal_rnorm_denominator(gx[i], gy[i]);
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = div_rn(gx[i], nrm[i]);
    const float n0 = median16(a);
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = div_rn(gy[i], nrm[i]);
    const float n1 = median16(a);
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = div_rn(-1.f, nrm[i]);
    const float n2 = median16(a);
    norm_gt[(long long)b * 3 * hw + q] = n0;
    norm_gt[((long long)b * 3 + 1) * hw + q] = n1;
    norm_gt[((long long)b * 3 + 2) * hw + q] = n2;
    norm_mask[p] = div_rn(n0, n2) < 5.f && div_rn(n1, n2) < 5.f;
    valid_dense[p] = maxpool_nonzero(valid, vmode, flow, img, W, y, x);
    valid_sparse[p] = bilinear_is_one(valid, vmode, flow, img, H, W, h, w, y, x);
}

// From an already full-resolution GT [B,C,H,W] (C = 2: gradients, mask on each channel; C = 3: normals, mask on n_x/n_z and n_y/n_z)
__global__ __launch_bounds__(LOSS_NT) void k_loss_targets_full(const float* __restrict__ gt, int C, const void* __restrict__ valid,
                                                               int vmode, int B, int H, int W, float* __restrict__ out,
                                                               uint8_t* __restrict__ gt_mask, uint8_t* __restrict__ valid_dense,
                                                               uint8_t* __restrict__ valid_sparse) {
    const int h = H / 4, w = W / 4;
    const long long n = (long long)B * h * w;
    const long long p = (long long)blockIdx.x * LOSS_NT + threadIdx.x;
    if (p >= n) return;
    const int x = (int)(p % w), y = (int)((p / w) % h), b = (int)(p / ((long long)h * w));
    const long long hw = (long long)h * w, q = (long long)y * w + x;
    float m[3] = {0.f, 0.f, 1.f};
    for (int c = 0; c < C; ++c) {
        const float* src = gt + ((long long)b * C + c) * H * W;
        float a[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) a[4 * i + j] = src[(long long)(4 * y + i) * W + 4 * x + j];
        const float v = median16(a);
        out[((long long)b * C + c) * hw + q] = v;
        if (c == 0) m[0] = v;
        else if (c == 1) m[1] = v;
        else m[2] = v;
    }
    gt_mask[p] = C == 3 ? (div_rn(m[0], m[2]) < 5.f && div_rn(m[1], m[2]) < 5.f) : (m[0] < 5.f && m[1] < 5.f);
    const long long img = (long long)b * H * W;          // the valid mask is [B,1,H,W]
    valid_dense[p] = maxpool_nonzero(valid, vmode, nullptr, img, W, y, x);
    valid_sparse[p] = bilinear_is_one(valid, vmode, nullptr, img, H, W, h, w, y, x);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sequence_loss (train_stereo.py:94-135): slots [0, iters) = sum over the mask of |q - gt| + 1.2 |r - gt| per iteration, then
// init L1, mono L1, count, EPE sums (last q, last r, init), EPE < 1/3/5 counts (q, r), non-finite count
// ---------------------------------------------------------------------------------------------------------------------------------
struct SeqArgs {
    const float* preds;          // iteration i: q at preds + i * it_stride, r at + ref_off
    long long it_stride, ref_off;
    int iters;
    const float* gt;
    const void* valid;
    int vmode;
    const float* mono;
    const float* init;
    long long n;                 // B*H*W
    double* part;
};

__global__ __launch_bounds__(LOSS_NT) void k_sequence_loss(SeqArgs a) {
    __shared__ double sh[12][LOSS_NT / TCS_WAVE];
    const int S = a.iters + 13;
    double* out = a.part + (long long)blockIdx.x * S;
    const long long base = (long long)blockIdx.x * LOSS_NT * SEQ_PIX + threadIdx.x;
    float g[SEQ_PIX];
    bool m[SEQ_PIX], in[SEQ_PIX];
#pragma unroll
    for (int j = 0; j < SEQ_PIX; ++j) {
        const long long p = base + (long long)j * LOSS_NT;
        in[j] = p < a.n;
        g[j] = in[j] ? a.gt[p] : 0.f;
        m[j] = in[j] && valid_at(a.valid, a.vmode, a.gt, p) != 0.f;
    }
    int bad = 0;
    for (int it = 0; it < a.iters; ++it) {
        const float* q = a.preds + it * a.it_stride;
        const float* r = q + a.ref_off;
        double s[1] = {0.0};
#pragma unroll
        for (int j = 0; j < SEQ_PIX; ++j) {
            if (!in[j]) continue;
            const long long p = base + (long long)j * LOSS_NT;
            const float qv = q[p], rv = r[p];
            bad += !finite(qv) || !finite(rv);
            if (m[j]) s[0] += (double)(fabsf(qv - g[j]) + 1.2f * fabsf(rv - g[j]));
        }
        block_sum<1>(s, sh);
        if (threadIdx.x == 0) out[it] = s[0];
    }
    const float* q = a.preds + (a.iters - 1) * a.it_stride;
    const float* r = q + a.ref_off;
    double v[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < SEQ_PIX; ++j) {
        if (!in[j]) continue;
        const long long p = base + (long long)j * LOSS_NT;
        const float iv = a.init[p], mv = a.mono[p];
        bad += isnan(iv) || isnan(mv);
        if (!m[j]) continue;
        const float dq = q[p] - g[j], dr = r[p] - g[j], di = iv - g[j];
        const float eq = sqrt_rn(dq * dq), er = sqrt_rn(dr * dr), ei = sqrt_rn(di * di);
        v[0] += (double)fabsf(di);
        v[1] += (double)fabsf(mv - g[j]);
        v[2] += 1.0;
        v[3] += (double)eq;
        v[4] += (double)er;
        v[5] += (double)ei;
        v[6] += eq < 1.f;
        v[7] += eq < 3.f;
        v[8] += eq < 5.f;
        v[9] += er < 1.f;
        v[10] += er < 3.f;
        v[11] += er < 5.f;
    }
    block_sum<12>(v, sh);
    double fb[1] = {(double)bad};
    block_sum<1>(fb, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) out[a.iters + i] = v[i];
        out[a.iters + 12] = fb[0];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// init_loss (train_stereo.py:138-180): one thread per quarter pixel loops over the D candidates of cost_volume [B,D,h,w] (reads are
// coalesced along w1), the masked top-K in registers.  Slots: sum of phi_gt over the mask, mask count, the clipped top-K sum, the
// forward-mask count over all pixels, non-finite count.
// ---------------------------------------------------------------------------------------------------------------------------------
// The per-pixel geometry of init_loss (train_stereo.py:141-160) at quarter pixel p of [B,h,w]: the mask, the clipped index and its two
// gathered entries, phi_gt, and the +-1.5 exclusion window.  One definition for the forward and the backward: the backward's mask
// and hinge are the forward's, bit for bit.
struct InitPixel {
    bool mask;
    int x, df, i0, i1;           // the gathered entries col[i0] (weight 1 - t) and col[i1] (weight t)
    float fs, t, phi, lo, hi;
    const float* col;            // cost_volume[b, :, y, x], stride cs
    long long cs;
};

__device__ __forceinline__ InitPixel init_pixel(const float* __restrict__ cv, int D, const float* __restrict__ flow,
                                                const void* __restrict__ valid, int vmode, int H, int W, int h, int w, long long p) {
    InitPixel g;
    const int x = (int)(p % w), y = (int)((p / w) % h), b = (int)(p / ((long long)h * w));
    const long long img = (long long)b * H * W;
    const float fs = 0.25f * flow[img + (long long)(4 * y) * W + 4 * x];          // nearest, x scale
    const bool ok = bilinear_is_one(valid, vmode, flow, img, H, W, h, w, y, x) && sqrt_rn(fs * fs) < 175.f;
    const float dmax = (float)(D - 1);
    const float idx = (float)x - (-fs);
    g.mask = ok && idx >= 0.f && idx <= dmax;
    const float ic = fminf(fmaxf(idx, 0.f), dmax);
    g.col = cv + (long long)b * D * h * w + (long long)y * w + x;
    g.cs = (long long)h * w;
    g.x = x;
    g.fs = fs;
    g.df = (int)floorf(ic);
    g.t = ic - (float)g.df;
    g.i1 = min(max(g.df + 1, 0), D - 1);
    g.i0 = min(max(g.df, 0), D - 1);
    g.phi = g.t * g.col[g.i1 * g.cs] + (1.f - g.t) * g.col[g.i0 * g.cs];
    g.lo = ic - 1.5f;
    g.hi = ic + 1.5f;
    return g;
}

template <int K>
__global__ __launch_bounds__(LOSS_NT) void k_init_loss(const float* __restrict__ cv, int D, const float* __restrict__ flow,
                                                       const void* __restrict__ valid, int vmode, int B, int H, int W, float threshold,
                                                       double* __restrict__ part) {
    __shared__ double sh[5][LOSS_NT / TCS_WAVE];
    const int h = H / 4, w = W / 4;
    const long long n = (long long)B * h * w;
    const long long p = (long long)blockIdx.x * LOSS_NT + threadIdx.x;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < n) {
        const InitPixel g = init_pixel(cv, D, flow, valid, vmode, H, W, h, w, p);
        const bool mask = g.mask;
        const float* col = g.col;
        const long long cs = g.cs;
        const float phi = g.phi, lo = g.lo, hi = g.hi;
        float top[K];
#pragma unroll
        for (int j = 0; j < K; ++j) top[j] = -INFINITY;
        int bad = 0;
        for (int c = 0; c < D; ++c) {
            const float cvv = col[c * cs];
            bad += !finite(cvv);
            const float fc = (float)c;
            float val = ((fc >= lo && fc < hi) || !mask) ? 0.f : cvv;
#pragma unroll
            for (int j = 0; j < K; ++j) {                  // insertion into the descending list
                const float cur = top[j];
                const bool gt = val > cur;
                top[j] = gt ? val : cur;
                val = gt ? cur : val;
            }
        }
        if (mask) {
            v[0] = (double)phi;
            v[1] = 1.0;
#pragma unroll
            for (int j = 0; j < K; ++j) v[2] += (double)fmaxf((top[j] + threshold) - phi, 0.f);
        }
        v[3] = ((top[0] + 0.3f) - phi) > 0.f;
        v[4] = (double)bad;
    }
    block_sum<5>(v, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int i = 0; i < 5; ++i) part[(long long)blockIdx.x * 5 + i] = v[i];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// disp_grad_loss (train_stereo.py:41-64) and disp_normal_loss (:67-91) over all iterations: slots 3*i, 3*i+1, 3*i+2 = the masked sums of
// the gradient loss, the normal loss of -flow_q and of -flow_q_refine; then the two mask counts and the non-finite count.
// ---------------------------------------------------------------------------------------------------------------------------------
struct GradNormArgs {
    const float* grad_preds;     // iteration i at + i * grad_stride, [B,2,h,w]; NULL = no gradient loss
    long long grad_stride;
    const float* q_preds;        // iteration i: flow_q at + i * q_stride, flow_q_refine at + q_ref_off, [B,1,h,w]; NULL = no normal loss
    long long q_stride, q_ref_off;
    int iters;
    const float* grad_gt;
    const uint8_t* grad_mask;
    const uint8_t* grad_valid;
    const float* norm_gt;
    const uint8_t* norm_mask;
    const uint8_t* norm_valid;
    int B, h, w;
    double* part;
};

// 0.5 * mean_c |n - n_gt| + 0.5 * (1 - n . n_gt), n the normal of -flow at (y, x) (disp2disp_normal_xy)
__device__ __forceinline__ float normal_loss_at(const float* f, int h, int w, int y, int x, const float (&ng)[3]) {
    const float d00 = -f[(long long)y * w + x];
    const float d01 = -f[(long long)y * w + min(x + 1, w - 1)];
    const float d10 = -f[(long long)min(y + 1, h - 1) * w + x];
    const float gx = d01 - d00, gy = d10 - d00;
    const float nr = normal_rnorm_denominator(gx, gy);
    const float n0 = div_rn(gx, nr), n1 = div_rn(gy, nr), n2 = div_rn(-1.f, nr);
    const float l1 = div_rn((fabsf(n0 - ng[0]) + fabsf(n1 - ng[1])) + fabsf(n2 - ng[2]), 3.f);
    const float dot = (n0 * ng[0] + n1 * ng[1]) + n2 * ng[2];
    return 0.5f * l1 + 0.5f * (1.f - dot);
}

__global__ __launch_bounds__(LOSS_NT) void k_grad_normal_loss(GradNormArgs a) {
    __shared__ double sh[3][LOSS_NT / TCS_WAVE];
    const long long hw = (long long)a.h * a.w, n = (long long)a.B * hw;
    const long long p = (long long)blockIdx.x * LOSS_NT + threadIdx.x;
    const int S = 3 * a.iters + 3;
    double* out = a.part + (long long)blockIdx.x * S;
    const bool in = p < n;
    int x = 0, y = 0, b = 0;
    bool mg = false, mn = false;
    float gg[2] = {0.f, 0.f}, ng[3] = {0.f, 0.f, 0.f};
    if (in) {
        x = (int)(p % a.w);
        y = (int)((p / a.w) % a.h);
        b = (int)(p / hw);
        const long long q = (long long)y * a.w + x;
        if (a.grad_preds) {
            mg = a.grad_valid[p] && a.grad_mask[p];
            gg[0] = a.grad_gt[(long long)b * 2 * hw + q];
            gg[1] = a.grad_gt[((long long)b * 2 + 1) * hw + q];
        }
        if (a.q_preds) {
            mn = a.norm_valid[p] && a.norm_mask[p];
#pragma unroll
            for (int c = 0; c < 3; ++c) ng[c] = a.norm_gt[((long long)b * 3 + c) * hw + q];
        }
    }
    int bad = 0;
    for (int it = 0; it < a.iters; ++it) {
        double s[3] = {0.0, 0.0, 0.0};
        if (in && a.grad_preds) {
            const float* g = a.grad_preds + it * a.grad_stride + (long long)b * 2 * hw + (long long)y * a.w + x;
            const float g0 = g[0], g1 = g[hw];
            bad += !finite(g0) || !finite(g1);
            if (mg) s[0] = (double)((fabsf(g0 - gg[0]) + fabsf(g1 - gg[1])) / 2.f);
        }
        if (in && mn) {
            const float* fq = a.q_preds + it * a.q_stride + (long long)b * hw;
            s[1] = (double)normal_loss_at(fq, a.h, a.w, y, x, ng);
            s[2] = (double)normal_loss_at(fq + a.q_ref_off, a.h, a.w, y, x, ng);
        }
        block_sum<3>(s, sh);
        if (threadIdx.x == 0) {
            out[3 * it] = s[0];
            out[3 * it + 1] = s[1];
            out[3 * it + 2] = s[2];
        }
    }
    double c[3] = {(double)mg, (double)mn, (double)bad};
    block_sum<3>(c, sh);
    if (threadIdx.x == 0) {
        out[3 * a.iters] = c[0];
        out[3 * a.iters + 1] = c[1];
        out[3 * a.iters + 2] = c[2];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the finish: each wave sums one slot over its blocks (lane j: blocks j, j+64, ...; then a fixed shuffle tree), then thread 0 forms
// the losses and the metrics (the output order is TCS_LOSS_OUT_* in include/tcs_mi355.h)
// ---------------------------------------------------------------------------------------------------------------------------------
#define FIN_NT 1024
#define FIN_MAX_SLOTS (3 * TCS_LOSS_MAX_ITERS + 3 + TCS_LOSS_MAX_ITERS + 13 + 5)

struct FinishArgs {
    const double* part;
    int parts;
    int iters, k;
    int seq_blocks, init_blocks, gn_blocks;
    long long seq_off, init_off, gn_off;   // in doubles
    double quarter_pixels;
    double weights[TCS_LOSS_MAX_ITERS];
    double* out;
    float* out32;
    double* counts;              // [TCS_LOSS_NCOUNTS] mask counts for the backward kernels, or NULL
};

__global__ __launch_bounds__(FIN_NT) void k_loss_finish(FinishArgs a) {
    __shared__ double tot[FIN_MAX_SLOTS];
    const int S_seq = a.iters + 13, S_init = 5, S_gn = 3 * a.iters + 3;
    const int nslots = S_seq + S_init + S_gn;
    const int lane = threadIdx.x & (TCS_WAVE - 1), wid = threadIdx.x / TCS_WAVE;
    for (int s = wid; s < nslots; s += FIN_NT / TCS_WAVE) {
        const double* base;
        int nb, stride;
        if (s < S_seq) { base = a.part + a.seq_off + s; nb = (a.parts & TCS_LOSS_SEQ) ? a.seq_blocks : 0; stride = S_seq; }
        else if (s < S_seq + S_init) { base = a.part + a.init_off + (s - S_seq); nb = (a.parts & TCS_LOSS_INIT) ? a.init_blocks : 0; stride = S_init; }
        else { base = a.part + a.gn_off + (s - S_seq - S_init); nb = (a.parts & (TCS_LOSS_GRAD | TCS_LOSS_NORM)) ? a.gn_blocks : 0; stride = S_gn; }
        double t = 0.0;
        for (int i = lane; i < nb; i += TCS_WAVE) t += base[(long long)i * stride];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, TCS_WAVE);
        if (lane == 0) tot[s] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double o[TCS_LOSS_NOUT];
    for (int i = 0; i < TCS_LOSS_NOUT; ++i) o[i] = NAN;
    double flags = 0.0;
    const double* sq = tot;
    const double* in = tot + S_seq;
    const double* gn = tot + S_seq + S_init;
    if (a.parts & TCS_LOSS_SEQ) {
        const double cnt = sq[a.iters + 2];
        double l = 0.1 * (sq[a.iters] / cnt) + 0.1 * (sq[a.iters + 1] / cnt);
        for (int i = 0; i < a.iters; ++i) l += a.weights[i] * (sq[i] / cnt);
        o[TCS_LOSS_OUT_SEQ] = l;
        for (int i = 0; i < 9; ++i) o[TCS_LOSS_OUT_EPE + i] = sq[a.iters + 3 + i] / cnt;
        if (sq[a.iters + 12] != 0.0) flags += 1.0;
    }
    if (a.parts & TCS_LOSS_INIT) {
        const double cnt = in[1];
        const double g = 1.0 - in[0] / cnt, nm = in[2] / ((double)a.k * cnt);
        o[TCS_LOSS_OUT_INIT] = g + nm;
        o[TCS_LOSS_OUT_INIT_GT] = g;
        o[TCS_LOSS_OUT_INIT_NM] = nm;
        o[TCS_LOSS_OUT_FMR] = in[3] / a.quarter_pixels;
        if (in[4] != 0.0) flags += 2.0;
    }
    if (a.parts & TCS_LOSS_NORM) {
        const double cnt = gn[3 * a.iters + 1];
        double l = 0.0;
        for (int i = 0; i < a.iters; ++i) l += a.weights[i] * (gn[3 * i + 1] / cnt + 1.2 * (gn[3 * i + 2] / cnt));
        o[TCS_LOSS_OUT_NORM] = l;
    }
    if (a.parts & TCS_LOSS_GRAD) {
        const double cnt = gn[3 * a.iters];
        double l = 0.0;
        for (int i = 0; i < a.iters; ++i) l += a.weights[i] * (gn[3 * i] / cnt);
        o[TCS_LOSS_OUT_GRAD] = l;
        if (gn[3 * a.iters + 2] != 0.0) flags += 4.0;
    }
    o[TCS_LOSS_OUT_TOTAL] = o[TCS_LOSS_OUT_SEQ] + o[TCS_LOSS_OUT_INIT] + 0.25 * o[TCS_LOSS_OUT_NORM] + 5.0 * o[TCS_LOSS_OUT_GRAD];
    o[TCS_LOSS_OUT_FLAGS] = flags;
    for (int i = 0; i < TCS_LOSS_NOUT; ++i) a.out[i] = o[i];
    for (int i = 0; i < 5; ++i) a.out32[i] = (float)o[i];
    if (a.counts) {                                     // a part that is absent counts 0: its backward then writes zeros
        a.counts[TCS_LOSS_COUNT_SEQ] = (a.parts & TCS_LOSS_SEQ) ? sq[a.iters + 2] : 0.0;
        a.counts[TCS_LOSS_COUNT_INIT] = (a.parts & TCS_LOSS_INIT) ? in[1] : 0.0;
        a.counts[TCS_LOSS_COUNT_NORM] = (a.parts & TCS_LOSS_NORM) ? gn[3 * a.iters + 1] : 0.0;
        a.counts[TCS_LOSS_COUNT_GRAD] = (a.parts & TCS_LOSS_GRAD) ? gn[3 * a.iters] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The backward kernels.  Every loss is a masked mean, so a gradient is a sign or a short stencil times
// upstream * weight / count.  The upstream gradient (the five float32 of d/d out32: total, seq, init, norm, grad) and the counts (the
// finish's TCS_LOSS_COUNT_* vector) are read from device memory: no host synchronisation.  Coefficients are formed in fp64 and
// rounded once; a count of 0 (an empty mask) gives coefficient 0, never NaN.  Every output element is written exactly once by one
// thread, zeros included: no memset, no atomics, two backwards are bit-equal.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double inv_count(const double* counts, int which) {
    const double n = counts[which];
    return n > 0.0 ? 1.0 / n : 0.0;
}

// torch.sign / the backward of abs: 0 at 0 (and at NaN)
__device__ __forceinline__ float sign_of(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

struct SeqBwdArgs {
    const float* preds;          // as SeqArgs
    float* g_preds;              // same layout as preds, or NULL
    long long it_stride, ref_off;
    int iters;
    const float* gt;
    const void* valid;
    int vmode;
    const float* mono;
    const float* init;
    float* g_mono;               // or NULL
    float* g_init;               // or NULL
    long long n;
    const double* counts;
    const float* upstream;
    double weights[TCS_LOSS_MAX_ITERS];
};

// the forward's layout: SEQ_PIX pixels per thread, gt and mask read once into registers, iters x 2 + 2 maps read and written once
__global__ __launch_bounds__(LOSS_NT) void k_sequence_loss_bwd(SeqBwdArgs a) {
    const long long base = (long long)blockIdx.x * LOSS_NT * SEQ_PIX + threadIdx.x;
    const double c = ((double)a.upstream[TCS_LOSS_OUT_TOTAL] + (double)a.upstream[TCS_LOSS_OUT_SEQ]) * inv_count(a.counts, TCS_LOSS_COUNT_SEQ);
    float g[SEQ_PIX];
    bool m[SEQ_PIX], in[SEQ_PIX];
#pragma unroll
    for (int j = 0; j < SEQ_PIX; ++j) {
        const long long p = base + (long long)j * LOSS_NT;
        in[j] = p < a.n;
        g[j] = in[j] ? a.gt[p] : 0.f;
        m[j] = in[j] && valid_at(a.valid, a.vmode, a.gt, p) != 0.f;
    }
    if (a.g_preds)
        for (int it = 0; it < a.iters; ++it) {
            const float* q = a.preds + it * a.it_stride;
            float* gq = a.g_preds + it * a.it_stride;
            const float cq = (float)(c * a.weights[it]), cr = (float)(c * a.weights[it] * 1.2);
#pragma unroll
            for (int j = 0; j < SEQ_PIX; ++j) {
                if (!in[j]) continue;
                const long long p = base + (long long)j * LOSS_NT;
                const float qv = q[p], rv = q[a.ref_off + p];
                gq[p] = m[j] ? sign_of(qv - g[j]) * cq : 0.f;
                gq[a.ref_off + p] = m[j] ? sign_of(rv - g[j]) * cr : 0.f;
            }
        }
    const float c01 = (float)(c * 0.1);
#pragma unroll
    for (int j = 0; j < SEQ_PIX; ++j) {
        if (!in[j]) continue;
        const long long p = base + (long long)j * LOSS_NT;
        if (a.g_mono) a.g_mono[p] = m[j] ? sign_of(a.mono[p] - g[j]) * c01 : 0.f;
        if (a.g_init) a.g_init[p] = m[j] ? sign_of(a.init[p] - g[j]) * c01 : 0.f;
    }
}

struct GradNormBwdArgs {
    const float* grad_preds;     // as GradNormArgs; NULL = no gradient-loss backward
    float* g_grad;               // same layout as grad_preds
    long long grad_stride;
    const float* q_preds;        // NULL = no normal-loss backward
    float* g_q;                  // same layout as q_preds
    long long q_stride, q_ref_off;
    int iters;
    const float* grad_gt;
    const uint8_t* grad_mask;
    const uint8_t* grad_valid;
    const float* norm_gt;
    const uint8_t* norm_mask;
    const uint8_t* norm_valid;
    int B, h, w;
    const double* counts;
    const float* upstream;
    double weights[TCS_LOSS_MAX_ITERS];
};

// d(loss pixel)/d(gx, gy) of 0.5 * mean_c |n - n_gt| + 0.5 * (1 - n . n_gt), n = (gx, gy, -1) / sqrt(gx^2 + gy^2 + 1), at the loss pixel
// whose own / right / lower values of flow_q are f00, f01, f10 (gx = f00 - f01, gy = f00 - f10: the differences of -flow).  The signs
// come from the forward's fp32 normal (normal_loss_at's operations), the magnitudes are fp64.
__device__ __forceinline__ void normal_loss_dg(float f00, float f01, float f10, const float (&ng)[3], double& dgx, double& dgy) {
    const float d00 = -f00, d01 = -f01, d10 = -f10;
    const float gx = d01 - d00, gy = d10 - d00;
    const float nr = normal_rnorm_denominator(gx, gy);
    const float n0 = div_rn(gx, nr), n1 = div_rn(gy, nr), n2 = div_rn(-1.f, nr);
    const double a0 = (double)sign_of(n0 - ng[0]) / 6.0 - 0.5 * (double)ng[0];
    const double a1 = (double)sign_of(n1 - ng[1]) / 6.0 - 0.5 * (double)ng[1];
    const double a2 = (double)sign_of(n2 - ng[2]) / 6.0 - 0.5 * (double)ng[2];
    const double x = (double)gx, y = (double)gy;
    const double ir = 1.0 / sqrt((x * x + y * y) + 1.0);
    const double m0 = x * ir, m1 = y * ir, m2 = -ir;
    const double an = (a0 * m0 + a1 * m1) + a2 * m2;
    dgx = (a0 - an * m0) * ir;
    dgy = (a1 - an * m1) * ir;
}

// One thread per quarter pixel and iteration (blockIdx.y).  The normal loss is a gather: pixel (y, x) collects from the loss pixels (y, x), (y, x-1) and (y-1, x);
// at the last column / row the replicate pad makes the difference identically 0, so that term is absent.  The mask is the loss pixel's.
__global__ __launch_bounds__(LOSS_NT) void k_grad_normal_loss_bwd(GradNormBwdArgs a) {
    const long long hw = (long long)a.h * a.w, n = (long long)a.B * hw;
    const long long p = (long long)blockIdx.x * LOSS_NT + threadIdx.x;
    if (p >= n) return;
    const int x = (int)(p % a.w), y = (int)((p / a.w) % a.h), b = (int)(p / hw);
    const long long q = (long long)y * a.w + x;
    const int it = blockIdx.y;
    const double up0 = (double)a.upstream[TCS_LOSS_OUT_TOTAL];
    if (a.grad_preds) {
        const bool mg = a.grad_valid[p] && a.grad_mask[p];
        const float g0t = a.grad_gt[(long long)b * 2 * hw + q], g1t = a.grad_gt[((long long)b * 2 + 1) * hw + q];
        const double c = (5.0 * up0 + (double)a.upstream[TCS_LOSS_OUT_GRAD]) * inv_count(a.counts, TCS_LOSS_COUNT_GRAD) * 0.5;
        const long long o = it * a.grad_stride + (long long)b * 2 * hw + q;
        const float ci = (float)(c * a.weights[it]);
        a.g_grad[o] = mg ? sign_of(a.grad_preds[o] - g0t) * ci : 0.f;
        a.g_grad[o + hw] = mg ? sign_of(a.grad_preds[o + hw] - g1t) * ci : 0.f;
    }
    if (a.q_preds) {
        // loss pixels: 0 = (y, x), 1 = (y, x-1), 2 = (y-1, x)
        const bool has1 = x >= 1, has2 = y >= 1;
        const long long pl[3] = {p, has1 ? p - 1 : p, has2 ? p - a.w : p};
        bool mn[3];
        float ng[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = a.norm_valid[pl[k]] && a.norm_mask[pl[k]];
            const long long ql = pl[k] - (long long)b * hw;
#pragma unroll
            for (int c = 0; c < 3; ++c) ng[k][c] = a.norm_gt[((long long)b * 3 + c) * hw + ql];
        }
        mn[1] = mn[1] && has1;
        mn[2] = mn[2] && has2;
        const bool xin = x < a.w - 1, yin = y < a.h - 1;     // the loss pixel (y, x)'s own differences exist
        const int xr = min(x + 1, a.w - 1), yd = min(y + 1, a.h - 1), xl = max(x - 1, 0), yu = max(y - 1, 0);
        const double c = (0.25 * up0 + (double)a.upstream[TCS_LOSS_OUT_NORM]) * inv_count(a.counts, TCS_LOSS_COUNT_NORM);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const long long o = it * a.q_stride + r * a.q_ref_off + (long long)b * hw;
            const float* f = a.q_preds + o;
            const float fc = f[q];
            double s = 0.0, dgx, dgy;
            if (mn[0]) {
                normal_loss_dg(fc, f[(long long)y * a.w + xr], f[(long long)yd * a.w + x], ng[0], dgx, dgy);
                s += (xin ? dgx : 0.0) + (yin ? dgy : 0.0);
            }
            if (mn[1]) {                                 // (y, x-1): this pixel is its right neighbour
                normal_loss_dg(f[(long long)y * a.w + xl], fc, f[(long long)yd * a.w + xl], ng[1], dgx, dgy);
                s -= dgx;
            }
            if (mn[2]) {                                 // (y-1, x): this pixel is its lower neighbour
                normal_loss_dg(f[(long long)yu * a.w + x], f[(long long)yu * a.w + xr], fc, ng[2], dgx, dgy);
                s -= dgy;
            }
            a.g_q[o + q] = (float)(s * (c * a.weights[it] * (r ? 1.2 : 1.0)));
        }
    }
}

// One thread per quarter pixel walks its column as k_init_loss does, keeps the top-K with their indices (a strict > insertion: among
// equal values the lowest index comes first; a zero-filled candidate carries index -1 and receives nothing), and writes the whole
// column: -(1 - t) / N and -t / N on the two gathered entries, +1 / (K N) on every real top-K entry whose hinge is >= 0, 0 elsewhere.
template <int K>
__global__ __launch_bounds__(LOSS_NT) void k_init_loss_bwd(const float* __restrict__ cv, float* __restrict__ g_cv, int D,
                                                           const float* __restrict__ flow, const void* __restrict__ valid, int vmode,
                                                           int B, int H, int W, float threshold, const double* __restrict__ counts,
                                                           const float* __restrict__ upstream) {
    const int h = H / 4, w = W / 4;
    const long long n = (long long)B * h * w;
    const long long p = (long long)blockIdx.x * LOSS_NT + threadIdx.x;
    if (p >= n) return;
    const InitPixel g = init_pixel(cv, D, flow, valid, vmode, H, W, h, w, p);
    float* out = g_cv + (g.col - cv);
    if (!g.mask) {
        for (int c = 0; c < D; ++c) out[c * g.cs] = 0.f;
        return;
    }
    float top[K];
    int ti[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        top[j] = -INFINITY;
        ti[j] = -1;
    }
    for (int c = 0; c < D; ++c) {
        const float fc = (float)c;
        const bool excl = fc >= g.lo && fc < g.hi;
        float val = excl ? 0.f : g.col[c * g.cs];
        int vi = excl ? -1 : c;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float cur = top[j];
            const int ci = ti[j];
            const bool gt = val > cur;
            top[j] = gt ? val : cur;
            ti[j] = gt ? vi : ci;
            val = gt ? cur : val;
            vi = gt ? ci : vi;
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (!(((top[j] + threshold) - g.phi) >= 0.f)) ti[j] = -1;
    const double c0 = ((double)upstream[TCS_LOSS_OUT_TOTAL] + (double)upstream[TCS_LOSS_OUT_INIT]) * inv_count(counts, TCS_LOSS_COUNT_INIT);
    // the clipped index in fp64 around the forward's floor: x + fs is exact there
    const double t = fmin(fmax((double)g.x + (double)g.fs, 0.0), (double)(D - 1)) - (double)g.df;
    const double cnm = c0 / (double)K;
    for (int c = 0; c < D; ++c) {
        double v = 0.0;
        if (c == g.i0) v -= (1.0 - t) * c0;
        if (c == g.i1) v -= t * c0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (ti[j] == c) v += cnm;
        out[c * g.cs] = (float)v;
    }
}

struct LossLayout {
    int seq_blocks, init_blocks, gn_blocks;
    long long seq_off, init_off, gn_off, total;
};

LossLayout loss_layout(int B, int H, int W, int iters) {
    LossLayout L;
    const long long n = (long long)B * H * W, nq = (long long)B * (H / 4) * (W / 4);
    L.seq_blocks = tcs_cdiv(n, LOSS_NT * SEQ_PIX);
    L.init_blocks = tcs_cdiv(nq, LOSS_NT);
    L.gn_blocks = tcs_cdiv(nq, LOSS_NT);
    L.seq_off = 0;
    L.init_off = L.seq_off + (long long)L.seq_blocks * (iters + 13);
    L.gn_off = L.init_off + (long long)L.init_blocks * 5;
    L.total = L.gn_off + (long long)L.gn_blocks * (3 * iters + 3);
    return L;
}

bool shape_ok(int B, int H, int W) {
    return B > 0 && H >= 4 && W >= 4 && (long long)B * H * W <= 0x7fffffffLL;
}

int loss_finish_launch(const double* workspace, int parts, int B, int H, int W, int iters, int k, const double* loss_weights,
                       double* out, float* out32, double* counts, tcs_stream_t stream) {
    if (!workspace || !out || !out32 || parts <= 0 || parts > 15) return TCS_EINVAL;
    if (!shape_ok(B, H, W) || iters < 1 || iters > TCS_LOSS_MAX_ITERS || k < 1 || k > LOSS_MAX_K) return TCS_EINVAL;
    if ((parts & (TCS_LOSS_SEQ | TCS_LOSS_GRAD | TCS_LOSS_NORM)) && !loss_weights) return TCS_EINVAL;
    const LossLayout L = loss_layout(B, H, W, iters);
    FinishArgs a{};
    a.part = workspace;
    a.parts = parts;
    a.iters = iters;
    a.k = k;
    a.seq_blocks = L.seq_blocks;
    a.init_blocks = L.init_blocks;
    a.gn_blocks = L.gn_blocks;
    a.seq_off = L.seq_off;
    a.init_off = L.init_off;
    a.gn_off = L.gn_off;
    a.quarter_pixels = (double)B * (H / 4) * (W / 4);
    for (int i = 0; i < iters; ++i) a.weights[i] = loss_weights ? loss_weights[i] : 0.0;
    a.out = out;
    a.out32 = out32;
    a.counts = counts;
    hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(FIN_NT), 0, tcs_stream(stream), a);
    return tcs_launch_status();
}

}  // namespace

extern "C" {

size_t tcs_loss_workspace_bytes(int B, int H, int W, int iters) {
    if (!shape_ok(B, H, W) || iters < 1 || iters > TCS_LOSS_MAX_ITERS) return 0;
    return (size_t)loss_layout(B, H, W, iters).total * sizeof(double);
}

int tcs_loss_targets(const float* flow_gt, const void* valid, int valid_mode, int B, int H, int W, float* grad_gt, float* norm_gt,
                     uint8_t* grad_mask, uint8_t* norm_mask, uint8_t* valid_dense, uint8_t* valid_sparse, tcs_stream_t stream) {
    if (!flow_gt || !valid || !grad_gt || !norm_gt || !grad_mask || !norm_mask || !valid_dense || !valid_sparse) return TCS_EINVAL;
    if (!shape_ok(B, H, W) || valid_mode < 0 || valid_mode > 2) return TCS_EINVAL;
    const long long nq = (long long)B * (H / 4) * (W / 4);
    hipLaunchKernelGGL(k_loss_targets, dim3(tcs_cdiv(nq, LOSS_NT)), dim3(LOSS_NT), 0, tcs_stream(stream), flow_gt, valid, valid_mode,
                       B, H, W, grad_gt, norm_gt, grad_mask, norm_mask, valid_dense, valid_sparse);
    return tcs_launch_status();
}

int tcs_loss_targets_full(const float* gt, int C, const void* valid, int valid_mode, int B, int H, int W, float* out, uint8_t* gt_mask,
                          uint8_t* valid_dense, uint8_t* valid_sparse, tcs_stream_t stream) {
    if (!gt || !valid || !out || !gt_mask || !valid_dense || !valid_sparse) return TCS_EINVAL;
    if (!shape_ok(B, H, W) || (C != 2 && C != 3) || (valid_mode != 0 && valid_mode != 2)) return TCS_EINVAL;
    if ((long long)B * C * H * W > 0x7fffffffLL) return TCS_EUNSUPPORTED;
    const long long nq = (long long)B * (H / 4) * (W / 4);
    hipLaunchKernelGGL(k_loss_targets_full, dim3(tcs_cdiv(nq, LOSS_NT)), dim3(LOSS_NT), 0, tcs_stream(stream), gt, C, valid, valid_mode,
                       B, H, W, out, gt_mask, valid_dense, valid_sparse);
    return tcs_launch_status();
}

int tcs_sequence_loss(const float* preds, long long iter_stride, long long refine_offset, int iters, const float* flow_gt,
                      const void* valid, int valid_mode, const float* flow_mono, const float* flow_init, int B, int H, int W,
                      double* workspace, tcs_stream_t stream) {
    if (!preds || !flow_gt || !valid || !flow_mono || !flow_init || !workspace) return TCS_EINVAL;
    if (!shape_ok(B, H, W) || iters < 1 || iters > TCS_LOSS_MAX_ITERS || valid_mode < 0 || valid_mode > 2) return TCS_EINVAL;
    const LossLayout L = loss_layout(B, H, W, iters);
    SeqArgs a{preds, iter_stride, refine_offset, iters, flow_gt, valid, valid_mode, flow_mono, flow_init, (long long)B * H * W,
              workspace + L.seq_off};
    hipLaunchKernelGGL(k_sequence_loss, dim3(L.seq_blocks), dim3(LOSS_NT), 0, tcs_stream(stream), a);
    return tcs_launch_status();
}

int tcs_init_loss(const float* cost_volume, int D, const float* flow_gt, const void* valid, int valid_mode, int B, int H, int W, int k,
                  float threshold, int iters, double* workspace, tcs_stream_t stream) {
    if (!cost_volume || !flow_gt || !valid || !workspace) return TCS_EINVAL;
    if (!shape_ok(B, H, W) || D < 1 || k < 1 || k > LOSS_MAX_K || k > D || iters < 1 || iters > TCS_LOSS_MAX_ITERS) return TCS_EINVAL;
    if (valid_mode < 0 || valid_mode > 2) return TCS_EINVAL;
    if ((long long)B * D * (H / 4) * (W / 4) > 0x7fffffffLL) return TCS_EUNSUPPORTED;
    const LossLayout L = loss_layout(B, H, W, iters);
    double* part = workspace + L.init_off;
    const dim3 g(L.init_blocks), t(LOSS_NT);
    hipStream_t s = tcs_stream(stream);
#define TCS_INIT_K(KK) \
    case KK: hipLaunchKernelGGL(k_init_loss<KK>, g, t, 0, s, cost_volume, D, flow_gt, valid, valid_mode, B, H, W, threshold, part); break;
    switch (k) {
        TCS_INIT_K(1) TCS_INIT_K(2) TCS_INIT_K(3) TCS_INIT_K(4) TCS_INIT_K(5) TCS_INIT_K(6) TCS_INIT_K(7) TCS_INIT_K(8)
    }
#undef TCS_INIT_K
    return tcs_launch_status();
}

int tcs_grad_normal_loss(const float* grad_preds, long long grad_stride, const float* q_preds, long long q_stride, long long q_refine_offset,
                         int iters, const float* grad_gt, const uint8_t* grad_mask, const uint8_t* grad_valid, const float* norm_gt,
                         const uint8_t* norm_mask, const uint8_t* norm_valid, int B, int H, int W, double* workspace, tcs_stream_t stream) {
    if ((!grad_preds && !q_preds) || !workspace) return TCS_EINVAL;
    if (grad_preds && (!grad_gt || !grad_mask || !grad_valid)) return TCS_EINVAL;
    if (q_preds && (!norm_gt || !norm_mask || !norm_valid)) return TCS_EINVAL;
    if (!shape_ok(B, H, W) || iters < 1 || iters > TCS_LOSS_MAX_ITERS) return TCS_EINVAL;
    const LossLayout L = loss_layout(B, H, W, iters);
    GradNormArgs a{grad_preds, grad_stride, q_preds, q_stride, q_refine_offset, iters, grad_gt, grad_mask, grad_valid, norm_gt, norm_mask,
                   norm_valid, B, H / 4, W / 4, workspace + L.gn_off};
    hipLaunchKernelGGL(k_grad_normal_loss, dim3(L.gn_blocks), dim3(LOSS_NT), 0, tcs_stream(stream), a);
    return tcs_launch_status();
}

int tcs_loss_finish(const double* workspace, int parts, int B, int H, int W, int iters, int k, const double* loss_weights, double* out,
                    float* out32, tcs_stream_t stream) {
    return loss_finish_launch(workspace, parts, B, H, W, iters, k, loss_weights, out, out32, nullptr, stream);
}

int tcs_loss_finish_counts(const double* workspace, int parts, int B, int H, int W, int iters, int k, const double* loss_weights,
                           double* out, float* out32, double* counts, tcs_stream_t stream) {
    if (!counts) return TCS_EINVAL;
    return loss_finish_launch(workspace, parts, B, H, W, iters, k, loss_weights, out, out32, counts, stream);
}

int tcs_sequence_loss_bwd(const float* preds, long long iter_stride, long long refine_offset, int iters, const float* flow_gt,
                          const void* valid, int valid_mode, const float* flow_mono, const float* flow_init, int B, int H, int W,
                          const double* loss_weights, const double* counts, const float* upstream, float* grad_preds, float* grad_mono,
                          float* grad_init, tcs_stream_t stream) {
    if (!preds || !flow_gt || !valid || !flow_mono || !flow_init || !loss_weights || !counts || !upstream) return TCS_EINVAL;
    if (!grad_preds && !grad_mono && !grad_init) return TCS_EINVAL;
    if (!shape_ok(B, H, W) || iters < 1 || iters > TCS_LOSS_MAX_ITERS || valid_mode < 0 || valid_mode > 2) return TCS_EINVAL;
    SeqBwdArgs a{};
    a.preds = preds;
    a.g_preds = grad_preds;
    a.it_stride = iter_stride;
    a.ref_off = refine_offset;
    a.iters = iters;
    a.gt = flow_gt;
    a.valid = valid;
    a.vmode = valid_mode;
    a.mono = flow_mono;
    a.init = flow_init;
    a.g_mono = grad_mono;
    a.g_init = grad_init;
    a.n = (long long)B * H * W;
    a.counts = counts;
    a.upstream = upstream;
    for (int i = 0; i < iters; ++i) a.weights[i] = loss_weights[i];
    hipLaunchKernelGGL(k_sequence_loss_bwd, dim3(loss_layout(B, H, W, iters).seq_blocks), dim3(LOSS_NT), 0, tcs_stream(stream), a);
    return tcs_launch_status();
}

int tcs_init_loss_bwd(const float* cost_volume, int D, const float* flow_gt, const void* valid, int valid_mode, int B, int H, int W, int k,
                      float threshold, const double* counts, const float* upstream, float* grad_cost_volume, tcs_stream_t stream) {
    if (!cost_volume || !flow_gt || !valid || !counts || !upstream || !grad_cost_volume) return TCS_EINVAL;
    if (!shape_ok(B, H, W) || D < 1 || k < 1 || k > LOSS_MAX_K || k > D || valid_mode < 0 || valid_mode > 2) return TCS_EINVAL;
    if ((long long)B * D * (H / 4) * (W / 4) > 0x7fffffffLL) return TCS_EUNSUPPORTED;
    const dim3 g(tcs_cdiv((long long)B * (H / 4) * (W / 4), LOSS_NT)), t(LOSS_NT);
    hipStream_t s = tcs_stream(stream);
#define TCS_INIT_K(KK) \
    case KK: hipLaunchKernelGGL(k_init_loss_bwd<KK>, g, t, 0, s, cost_volume, grad_cost_volume, D, flow_gt, valid, valid_mode, B, H, W, \
                                threshold, counts, upstream); break;
    switch (k) {
        TCS_INIT_K(1) TCS_INIT_K(2) TCS_INIT_K(3) TCS_INIT_K(4) TCS_INIT_K(5) TCS_INIT_K(6) TCS_INIT_K(7) TCS_INIT_K(8)
    }
#undef TCS_INIT_K
    return tcs_launch_status();
}

int tcs_grad_normal_loss_bwd(const float* grad_preds, long long grad_stride, const float* q_preds, long long q_stride,
                             long long q_refine_offset, int iters, const float* grad_gt, const uint8_t* grad_mask, const uint8_t* grad_valid,
                             const float* norm_gt, const uint8_t* norm_mask, const uint8_t* norm_valid, int B, int H, int W,
                             const double* loss_weights, const double* counts, const float* upstream, float* grad_grad_preds,
                             float* grad_q_preds, tcs_stream_t stream) {
    if ((!grad_preds && !q_preds) || !loss_weights || !counts || !upstream) return TCS_EINVAL;
    if (grad_preds && (!grad_gt || !grad_mask || !grad_valid || !grad_grad_preds)) return TCS_EINVAL;
    if (q_preds && (!norm_gt || !norm_mask || !norm_valid || !grad_q_preds)) return TCS_EINVAL;
    if (!shape_ok(B, H, W) || iters < 1 || iters > TCS_LOSS_MAX_ITERS) return TCS_EINVAL;
    GradNormBwdArgs a{};
    a.grad_preds = grad_preds;
    a.g_grad = grad_grad_preds;
    a.grad_stride = grad_stride;
    a.q_preds = q_preds;
    a.g_q = grad_q_preds;
    a.q_stride = q_stride;
    a.q_ref_off = q_refine_offset;
    a.iters = iters;
    a.grad_gt = grad_gt;
    a.grad_mask = grad_mask;
    a.grad_valid = grad_valid;
    a.norm_gt = norm_gt;
    a.norm_mask = norm_mask;
    a.norm_valid = norm_valid;
    a.B = B;
    a.h = H / 4;
    a.w = W / 4;
    a.counts = counts;
    a.upstream = upstream;
    for (int i = 0; i < iters; ++i) a.weights[i] = loss_weights[i];
    hipLaunchKernelGGL(k_grad_normal_loss_bwd, dim3(loss_layout(B, H, W, iters).gn_blocks, iters), dim3(LOSS_NT), 0, tcs_stream(stream), a);
    return tcs_launch_status();
}

}  // extern "C"
