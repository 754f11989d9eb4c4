// The gate arithmetic of the reference's recurrent cells (core/update.py: ConvGRU :81-85, Lightfuse :30-34, HiddenstateUpdater
// :62-66) as two differentiable stages around the cell's second convolution, one launch forward and one backward each
// (tcs_mi355/train_ops.py):
//
//   reset :  r = sigmoid(r_pre + cr)                          rh    = r * h
//   update:  z = sigmoid(z_pre + cz), q = tanh(q_pre + cq)    h_new = (1 - z) h + z q     (ConvGRU)
//                                                             h_new = z h + (1 - z) q     (Lightfuse, HiddenstateUpdater: KEEP)
//
// Pure streaming work: every thread owns V consecutive floats of one batch element (V = 4, 16-byte loads and stores, when the
// element count per batch element, every batch stride and every base address allow it; V = 1 otherwise), reads each input plane
// once and writes each wanted output once.  No LDS, no atomics, no memset.  The inputs are views: each has its own batch stride in
// elements (chunk / split views of a wider convolution output are read in place); outputs are contiguous.  The grid is sized by
// the element count, `per_n` blocks for each batch element, so nothing is capped or grid-strided.
//
// The backward kernels recompute z, r and q from the inputs.  Both a gate and its complement come from one exp of -|x|, so 1 - z is
// never formed by a subtraction that cancels, and 1 - q^2 is 4 e / (1 + e)^2 with e = exp(-2|x|): |x| = 100 gives finite values and
// gradients that are zero, never inf * 0.
#include "tcs_common.h"

namespace {

constexpr int GATE_THREADS = 256;

template <int V> struct Pack { float v[V]; };

template <int V> __device__ __forceinline__ Pack<V> gate_load(const float* __restrict__ p) {
    Pack<V> r;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}

// a context term: NULL means zero
template <int V> __device__ __forceinline__ Pack<V> gate_load_ctx(const float* __restrict__ base, long long off) {
    if (base) return gate_load<V>(base + off);
    Pack<V> r;
#pragma unroll
    for (int j = 0; j < V; ++j) r.v[j] = 0.0f;
    return r;
}

template <int V> __device__ __forceinline__ void gate_store(float* __restrict__ p, const Pack<V>& r) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else *p = r.v[0];
}

// sigmoid(x) and 1 - sigmoid(x) = sigmoid(-x), each to a few ulp of itself: e = exp(-|x|) lies in [0, 1] and never overflows
struct Gate { float on, off; };
__device__ __forceinline__ Gate gate_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    const float big = 1.0f / (1.0f + e), small = e * big;
    Gate g;
    g.on = x >= 0.0f ? big : small;
    g.off = x >= 0.0f ? small : big;
    return g;
}

// 1 - tanh(x)^2 without the cancellation of 1 - q * q
__device__ __forceinline__ float gate_sech2(float x) {
    const float e = expf(-2.0f * fabsf(x)), d = 1.0f + e;
    return 4.0f * e / (d * d);
}

// this thread's offset inside its batch element, or -1 when it has none; n is the batch element
template <int V> __device__ __forceinline__ long long gate_index(long long chw, int per_n, int& n) {
    n = (int)(blockIdx.x / (unsigned)per_n);
    const long long i = ((long long)(blockIdx.x - (unsigned)n * (unsigned)per_n) * GATE_THREADS + threadIdx.x) * V;
    return i < chw ? i : -1;
}

template <int V>
__global__ __launch_bounds__(GATE_THREADS) void k_gru_reset(const float* __restrict__ r_pre, long long s_r, const float* __restrict__ h,
                                                            long long s_h, const float* __restrict__ cr, long long s_c, long long chw,
                                                            int per_n, float* __restrict__ rh) {
    int n;
    const long long i = gate_index<V>(chw, per_n, n);
    if (i < 0) return;
    const Pack<V> a = gate_load<V>(r_pre + n * s_r + i), hv = gate_load<V>(h + n * s_h + i), c = gate_load_ctx<V>(cr, n * s_c + i);
    Pack<V> o;
#pragma unroll
    for (int j = 0; j < V; ++j) o.v[j] = gate_sigmoid(a.v[j] + c.v[j]).on * hv.v[j];
    gate_store<V>(rh + n * chw + i, o);
}

// d r_pre = d cr = g h r (1 - r),  d h = g r
template <int V>
__global__ __launch_bounds__(GATE_THREADS) void k_gru_reset_bwd(const float* __restrict__ r_pre, long long s_r, const float* __restrict__ h,
                                                                long long s_h, const float* __restrict__ cr, long long s_c,
                                                                const float* __restrict__ grad, long long chw, int per_n,
                                                                float* __restrict__ g_pre, float* __restrict__ g_h) {
    int n;
    const long long i = gate_index<V>(chw, per_n, n);
    if (i < 0) return;
    const long long o = n * chw + i;
    const Pack<V> a = gate_load<V>(r_pre + n * s_r + i), c = gate_load_ctx<V>(cr, n * s_c + i), g = gate_load<V>(grad + o);
    Gate r[V];
#pragma unroll
    for (int j = 0; j < V; ++j) r[j] = gate_sigmoid(a.v[j] + c.v[j]);
    if (g_pre) {                                            // h is read for this gradient only
        const Pack<V> hv = gate_load<V>(h + n * s_h + i);
        Pack<V> d;
#pragma unroll
        for (int j = 0; j < V; ++j) d.v[j] = g.v[j] * hv.v[j] * (r[j].on * r[j].off);
        gate_store<V>(g_pre + o, d);
    }
    if (g_h) {
        Pack<V> d;
#pragma unroll
        for (int j = 0; j < V; ++j) d.v[j] = g.v[j] * r[j].on;
        gate_store<V>(g_h + o, d);
    }
}

template <int V, bool KEEP>
__global__ __launch_bounds__(GATE_THREADS) void k_gru_update(const float* __restrict__ z_pre, long long s_z, const float* __restrict__ q_pre,
                                                             long long s_q, const float* __restrict__ h, long long s_h,
                                                             const float* __restrict__ cz, long long s_cz, const float* __restrict__ cq,
                                                             long long s_cq, long long chw, int per_n, float* __restrict__ h_new) {
    int n;
    const long long i = gate_index<V>(chw, per_n, n);
    if (i < 0) return;
    const Pack<V> a = gate_load<V>(z_pre + n * s_z + i), b = gate_load<V>(q_pre + n * s_q + i), hv = gate_load<V>(h + n * s_h + i);
    const Pack<V> ca = gate_load_ctx<V>(cz, n * s_cz + i), cb = gate_load_ctx<V>(cq, n * s_cq + i);
    Pack<V> o;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const Gate z = gate_sigmoid(a.v[j] + ca.v[j]);
        const float q = tanhf(b.v[j] + cb.v[j]);
        const float wh = KEEP ? z.on : z.off, wq = KEEP ? z.off : z.on;        // the weights of h and of q
        o.v[j] = wh * hv.v[j] + wq * q;
    }
    gate_store<V>(h_new + n * chw + i, o);
}

// with wq the weight of q (z for ConvGRU, 1 - z with KEEP) and wh = 1 - wq the weight of h:
//   d q_pre = d cq = g wq (1 - q^2),   d h = g wh,   d z_pre = d cz = +-g (q - h) z (1 - z)   (- with KEEP)
template <int V, bool KEEP>
__global__ __launch_bounds__(GATE_THREADS) void k_gru_update_bwd(const float* __restrict__ z_pre, long long s_z,
                                                                 const float* __restrict__ q_pre, long long s_q, const float* __restrict__ h,
                                                                 long long s_h, const float* __restrict__ cz, long long s_cz,
                                                                 const float* __restrict__ cq, long long s_cq, const float* __restrict__ grad,
                                                                 long long chw, int per_n, float* __restrict__ g_z, float* __restrict__ g_q,
                                                                 float* __restrict__ g_h) {
    int n;
    const long long i = gate_index<V>(chw, per_n, n);
    if (i < 0) return;
    const long long o = n * chw + i;
    const Pack<V> a = gate_load<V>(z_pre + n * s_z + i), ca = gate_load_ctx<V>(cz, n * s_cz + i), g = gate_load<V>(grad + o);
    Gate z[V];
#pragma unroll
    for (int j = 0; j < V; ++j) z[j] = gate_sigmoid(a.v[j] + ca.v[j]);
    if (g_z || g_q) {                                       // q_pre and cq are read for these two only, h for d z_pre only
        const Pack<V> b = gate_load<V>(q_pre + n * s_q + i), cb = gate_load_ctx<V>(cq, n * s_cq + i);
        if (g_z) {
            const Pack<V> hv = gate_load<V>(h + n * s_h + i);
            Pack<V> d;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float diff = KEEP ? hv.v[j] - tanhf(b.v[j] + cb.v[j]) : tanhf(b.v[j] + cb.v[j]) - hv.v[j];
                d.v[j] = g.v[j] * diff * (z[j].on * z[j].off);
            }
            gate_store<V>(g_z + o, d);
        }
        if (g_q) {
            Pack<V> d;
#pragma unroll
            for (int j = 0; j < V; ++j) d.v[j] = g.v[j] * (KEEP ? z[j].off : z[j].on) * gate_sech2(b.v[j] + cb.v[j]);
            gate_store<V>(g_q + o, d);
        }
    }
    if (g_h) {
        Pack<V> d;
#pragma unroll
        for (int j = 0; j < V; ++j) d.v[j] = g.v[j] * (KEEP ? z[j].on : z[j].off);
        gate_store<V>(g_h + o, d);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct GateGrid {
    long long chw;
    int per_n, blocks, vec;
};

// sizes and the grid; TCS_EINVAL for a non-positive size, TCS_EUNSUPPORTED for more than 2^31 - 1 blocks
int gate_grid(int B, int C, int H, int W, GateGrid& gg) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return TCS_EINVAL;
    gg.chw = (long long)C * H * W;
    gg.per_n = gg.blocks = gg.vec = 0;
    return TCS_OK;
}

// an input view: its batch stride must step over a whole batch element
bool gate_stride_ok(const float* p, long long stride, const GateGrid& gg) { return !p || stride >= gg.chw; }

struct GateAlign {
    uintptr_t bits = 0;
    void ptr(const void* p) { bits |= (uintptr_t)p; }                        // NULL adds nothing
    void view(const float* p, long long stride) { if (p) bits |= (uintptr_t)p | (uintptr_t)(stride * 4); }
};

// 16-byte accesses when the element count per batch element, every batch stride and every base address are multiples of 16 bytes
int gate_finish(GateGrid& gg, int B, const GateAlign& al) {
    gg.vec = (gg.chw % 4 == 0 && (al.bits & 15) == 0) ? 4 : 1;
    const long long per_n = (gg.chw / gg.vec + GATE_THREADS - 1) / GATE_THREADS, blocks = per_n * B;
    if (blocks > 0x7fffffffLL) return TCS_EUNSUPPORTED;
    gg.per_n = (int)per_n;
    gg.blocks = (int)blocks;
    return TCS_OK;
}

}  // namespace

extern "C" {

int tcs_gru_reset(const float* r_pre, long long r_pre_stride, const float* h, long long h_stride, const float* cr, long long cr_stride,
                  int B, int C, int H, int W, float* rh, tcs_stream_t stream) {
    GateGrid gg;
    if (int rc = gate_grid(B, C, H, W, gg)) return rc;
    if (!r_pre || !h || !rh) return TCS_EINVAL;
    if (!gate_stride_ok(r_pre, r_pre_stride, gg) || !gate_stride_ok(h, h_stride, gg) || !gate_stride_ok(cr, cr_stride, gg)) return TCS_EINVAL;
    GateAlign al;
    al.view(r_pre, r_pre_stride); al.view(h, h_stride); al.view(cr, cr_stride); al.ptr(rh);
    if (int rc = gate_finish(gg, B, al)) return rc;
    auto k = gg.vec == 4 ? k_gru_reset<4> : k_gru_reset<1>;
    hipLaunchKernelGGL(k, dim3(gg.blocks), dim3(GATE_THREADS), 0, tcs_stream(stream), r_pre, r_pre_stride, h, h_stride, cr, cr_stride,
                       gg.chw, gg.per_n, rh);
    return tcs_launch_status();
}

int tcs_gru_reset_backward(const float* r_pre, long long r_pre_stride, const float* h, long long h_stride, const float* cr,
                           long long cr_stride, const float* grad_rh, int B, int C, int H, int W, float* grad_r_pre, float* grad_h,
                           tcs_stream_t stream) {
    GateGrid gg;
    if (int rc = gate_grid(B, C, H, W, gg)) return rc;
    if (!r_pre || !grad_rh || (!grad_r_pre && !grad_h) || (grad_r_pre && !h)) return TCS_EINVAL;
    if (!gate_stride_ok(r_pre, r_pre_stride, gg) || !gate_stride_ok(h, h_stride, gg) || !gate_stride_ok(cr, cr_stride, gg)) return TCS_EINVAL;
    GateAlign al;
    al.view(r_pre, r_pre_stride); al.view(h, h_stride); al.view(cr, cr_stride); al.ptr(grad_rh); al.ptr(grad_r_pre); al.ptr(grad_h);
    if (int rc = gate_finish(gg, B, al)) return rc;
    auto k = gg.vec == 4 ? k_gru_reset_bwd<4> : k_gru_reset_bwd<1>;
    hipLaunchKernelGGL(k, dim3(gg.blocks), dim3(GATE_THREADS), 0, tcs_stream(stream), r_pre, r_pre_stride, h, h_stride, cr, cr_stride,
                       grad_rh, gg.chw, gg.per_n, grad_r_pre, grad_h);
    return tcs_launch_status();
}

int tcs_gru_update(const float* z_pre, long long z_pre_stride, const float* q_pre, long long q_pre_stride, const float* h,
                   long long h_stride, const float* cz, long long cz_stride, const float* cq, long long cq_stride, int z_keeps_h, int B,
                   int C, int H, int W, float* h_new, tcs_stream_t stream) {
    GateGrid gg;
    if (int rc = gate_grid(B, C, H, W, gg)) return rc;
    if (!z_pre || !q_pre || !h || !h_new) return TCS_EINVAL;
    if (!gate_stride_ok(z_pre, z_pre_stride, gg) || !gate_stride_ok(q_pre, q_pre_stride, gg) || !gate_stride_ok(h, h_stride, gg) ||
        !gate_stride_ok(cz, cz_stride, gg) || !gate_stride_ok(cq, cq_stride, gg))
        return TCS_EINVAL;
    GateAlign al;
    al.view(z_pre, z_pre_stride); al.view(q_pre, q_pre_stride); al.view(h, h_stride); al.view(cz, cz_stride); al.view(cq, cq_stride);
    al.ptr(h_new);
    if (int rc = gate_finish(gg, B, al)) return rc;
    auto k = gg.vec == 4 ? (z_keeps_h ? k_gru_update<4, true> : k_gru_update<4, false>)
                         : (z_keeps_h ? k_gru_update<1, true> : k_gru_update<1, false>);
    hipLaunchKernelGGL(k, dim3(gg.blocks), dim3(GATE_THREADS), 0, tcs_stream(stream), z_pre, z_pre_stride, q_pre, q_pre_stride, h, h_stride,
                       cz, cz_stride, cq, cq_stride, gg.chw, gg.per_n, h_new);
    return tcs_launch_status();
}

int tcs_gru_update_backward(const float* z_pre, long long z_pre_stride, const float* q_pre, long long q_pre_stride, const float* h,
                            long long h_stride, const float* cz, long long cz_stride, const float* cq, long long cq_stride,
                            const float* grad_h_new, int z_keeps_h, int B, int C, int H, int W, float* grad_z_pre, float* grad_q_pre,
                            float* grad_h, tcs_stream_t stream) {
    GateGrid gg;
    if (int rc = gate_grid(B, C, H, W, gg)) return rc;
    if (!z_pre || !grad_h_new || (!grad_z_pre && !grad_q_pre && !grad_h)) return TCS_EINVAL;
    if (((grad_z_pre || grad_q_pre) && !q_pre) || (grad_z_pre && !h)) return TCS_EINVAL;
    if (!gate_stride_ok(z_pre, z_pre_stride, gg) || !gate_stride_ok(q_pre, q_pre_stride, gg) || !gate_stride_ok(h, h_stride, gg) ||
        !gate_stride_ok(cz, cz_stride, gg) || !gate_stride_ok(cq, cq_stride, gg))
        return TCS_EINVAL;
    GateAlign al;
    al.view(z_pre, z_pre_stride); al.view(q_pre, q_pre_stride); al.view(h, h_stride); al.view(cz, cz_stride); al.view(cq, cq_stride);
    al.ptr(grad_h_new); al.ptr(grad_z_pre); al.ptr(grad_q_pre); al.ptr(grad_h);
    if (int rc = gate_finish(gg, B, al)) return rc;
    auto k = gg.vec == 4 ? (z_keeps_h ? k_gru_update_bwd<4, true> : k_gru_update_bwd<4, false>)
                         : (z_keeps_h ? k_gru_update_bwd<1, true> : k_gru_update_bwd<1, false>);
    hipLaunchKernelGGL(k, dim3(gg.blocks), dim3(GATE_THREADS), 0, tcs_stream(stream), z_pre, z_pre_stride, q_pre, q_pre_stride, h, h_stride,
                       cz, cz_stride, cq, cq_stride, grad_h_new, gg.chw, gg.per_n, grad_z_pre, grad_q_pre, grad_h);
    return tcs_launch_status();
}

}  // extern "C"
