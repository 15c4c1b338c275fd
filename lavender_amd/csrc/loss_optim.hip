// Cross-entropy (fused forward + in-place logit gradient) and the flat-arena optimizer kernels.  All HBM-bound.
#include "common.h"
#include <math.h>
#include <stdlib.h>
#include "../../include/lavender_hip.h"

// ---- cross entropy, ignore_index = -1 (agent.py:72; main_pretrain_mlm.py:158-163) ---------------------
// one 256-thread block per row; online (max, sum-exp) in a single read, then one write pass
__global__ __launch_bounds__(256) void ce_kernel(int rows, int V, bf16_t* logits, long ld, const int64_t* labels, float* loss_sum,
                                                float grad_scale, int write_grad) {
    __shared__ float sm[8], ss[8];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bf16_t* x = logits + (long)row * ld;
    const long label = labels[row];
    const int nchunk = (int)(ld / 8);
    if (label < 0) {                                       // unlabelled row: zero gradient, no loss
        if (write_grad)
            for (int c = tid; c < nchunk; c += 256) *(uint4*)(x + c * 8) = make_uint4(0, 0, 0, 0);
        return;
    }
    float m = -INFINITY, s = 0.f;
    for (int c = tid; c < nchunk; c += 256) {
        float v[8];
        uint4 u = *(const uint4*)(x + c * 8);
        unpack8(u, v);
        float cm = -INFINITY;
#pragma unroll
        for (int k = 0; k < 8; ++k) { if (c * 8 + k >= V) v[k] = -INFINITY; cm = fmaxf(cm, v[k]); }
        if (cm > m) { s *= __expf(m - cm); m = cm; }
#pragma unroll
        for (int k = 0; k < 8; ++k) s += __expf(v[k] - m);
    }
    // wave then block reduction of (m, s)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        const float mn = fmaxf(m, m2);
        s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - mn));
        m = mn;
    }
    if (lane == 0) { sm[wave] = m; ss[wave] = s; }
    __syncthreads();
    float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    float S = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) S += ss[w] * __expf(sm[w] - M);
    const float lse = M + __logf(S);
    if (tid == 0) {
        atomicAdd(loss_sum, lse - bf2f(x[label]));
        atomicAdd(loss_sum + 1, 1.0f);
    }
    if (!write_grad) return;
    __syncthreads();                                       // x[label] read before anybody overwrites it
    for (int c = tid; c < nchunk; c += 256) {
        float v[8];
        uint4 u = *(const uint4*)(x + c * 8);
        unpack8(u, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int col = c * 8 + k;
            float g = col < V ? __expf(v[k] - lse) : 0.f;
            if (col == label) g -= 1.f;
            v[k] = g * grad_scale;
        }
        *(uint4*)(x + c * 8) = pack8(v);
    }
}

extern "C" int lav_cross_entropy_fwd_bwd(void* stream, int rows, int V, void* logits, long ld, const int64_t* labels, float* loss_sum,
                                         float grad_scale, int write_grad) {
    LAV_REQUIRE(rows > 0 && V > 0 && logits && labels && loss_sum, "lav_cross_entropy_fwd_bwd: bad arguments");
    LAV_REQUIRE(ld % 8 == 0 && ld >= V, "lav_cross_entropy_fwd_bwd: ld must be a multiple of 8 and >= V");
    hipLaunchKernelGGL(ce_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, rows, V, (bf16_t*)logits, ld, labels, loss_sum, grad_scale, write_grad);
    return lav_check_launch("lav_cross_entropy_fwd_bwd");
}

// fp32 logits, few classes (the (B, O) video-text matching scores): one wave per row, same contract as ce_kernel
__global__ __launch_bounds__(256) void ce_f32_kernel(int rows, int V, float* logits, long ld, const int64_t* labels, float* loss_sum,
                                                    float grad_scale, int write_grad) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* x = logits + (long)row * ld;
    const long label = labels[row];
    if (label < 0) {
        if (write_grad)
            for (int c = lane; c < V; c += 64) x[c] = 0.f;
        return;
    }
    float m = -INFINITY;
    for (int c = lane; c < V; c += 64) m = fmaxf(m, x[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < V; c += 64) s += __expf(x[c] - m);
    s = wave_sum(s);
    const float lse = m + __logf(s);
    const float xl = x[label];
    if (lane == 0) {
        atomicAdd(loss_sum, lse - xl);
        atomicAdd(loss_sum + 1, 1.0f);
    }
    if (!write_grad) return;
    for (int c = lane; c < V; c += 64) x[c] = (__expf(x[c] - lse) - (c == label ? 1.f : 0.f)) * grad_scale;
}

extern "C" int lav_cross_entropy_f32_fwd_bwd(void* stream, int rows, int V, float* logits, long ld, const int64_t* labels,
                                             float* loss_sum, float grad_scale, int write_grad) {
    LAV_REQUIRE(rows > 0 && V > 0 && ld >= V && logits && labels && loss_sum, "lav_cross_entropy_f32_fwd_bwd: bad arguments");
    hipLaunchKernelGGL(ce_f32_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, rows, V, logits, ld, labels, loss_sum,
                       grad_scale, write_grad);
    return lav_check_launch("lav_cross_entropy_f32_fwd_bwd");
}

// ---- captioning loss (model_for_captioning.py:10-37 on the labelled rows, main_caption.py:225-230) ------------------------------------
// label smoothing as the KL divergence to q (q_t = 1 - eps, q_c = eps / (V - 1)), "drop the worst" rows, the arg-max accuracy read-out and the
// in-place logit gradient.  One 256-thread block per row, the passes of ce_kernel: one read for (max, sum-exp, sum of logits, arg-max), one
// read + write for the gradient.  With the selection on, the gradient pass is a launch of its own behind the row losses (cap_select_kernel).
// No atomics anywhere: the four totals come from one block that adds the per-row results in a fixed order (bit-identical run to run).
struct CapArgs {
    int rows, V, k;
    bf16_t* logits; long ld; const int64_t* labels;
    float eps, C, q_other, scale;                          // C(eps, V); eps / (V - 1); 1 / k
    float* row_loss; float* row_lse; int32_t* correct; int32_t* kept; float* out;
};

__device__ __forceinline__ void cap_zero_row(bf16_t* x, int nchunk, int tid) {
    for (int c = tid; c < nchunk; c += 256) *(uint4*)(x + c * 8) = make_uint4(0, 0, 0, 0);
}

// x <- (softmax(x) - q) * scale on the V valid columns, 0 on the padding columns
__device__ __forceinline__ void cap_grad_row(bf16_t* x, int nchunk, int V, long label, float lse, float q_target, float q_other, float scale, int tid) {
    for (int c = tid; c < nchunk; c += 256) {
        float v[8];
        uint4 u = *(const uint4*)(x + c * 8);
        unpack8(u, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int col = c * 8 + k;
            const float g = col < V ? __expf(v[k] - lse) - (col == label ? q_target : q_other) : 0.f;
            v[k] = g * scale;
        }
        *(uint4*)(x + c * 8) = pack8(v);
    }
}

// FUSED: no selection, every labelled row is kept -- row results and (write_grad) the gradient in one launch
template <bool FUSED>
__global__ __launch_bounds__(256) void cap_row_kernel(CapArgs a, int write_grad) {
    __shared__ float sm[4], ss[4], sx[4], sb[4];
    __shared__ int si[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bf16_t* x = a.logits + (long)row * a.ld;
    const long label = a.labels[row];
    const int nchunk = (int)(a.ld / 8), V = a.V;
    if (label < 0 || label >= V) {                         // unlabelled (a label outside [0, V) is never used as a column)
        if (tid == 0) { a.row_loss[row] = 0.f; a.row_lse[row] = 0.f; a.correct[row] = 0; a.kept[row] = 0; }
        if (FUSED && write_grad) cap_zero_row(x, nchunk, tid);
        return;
    }
    float m = -INFINITY, s = 0.f, sum = 0.f, best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int c = tid; c < nchunk; c += 256) {
        float v[8];
        uint4 u = *(const uint4*)(x + c * 8);
        unpack8(u, v);
        float cm = -INFINITY;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int col = c * 8 + k;
            if (col >= V) v[k] = -INFINITY; else sum += v[k];
            cm = fmaxf(cm, v[k]);
            if (v[k] > best) { best = v[k]; bidx = col; }  // columns ascend within a thread: strict > keeps the lowest index
        }
        if (cm > m) { s *= __expf(m - cm); m = cm; }
#pragma unroll
        for (int k = 0; k < 8; ++k) s += __expf(v[k] - m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64), b2 = __shfl_xor(best, o, 64);
        const int i2 = __shfl_xor(bidx, o, 64);
        const float mn = fmaxf(m, m2);
        s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - mn));
        m = mn;
        sum += __shfl_xor(sum, o, 64);
        if (b2 > best || (b2 == best && i2 < bidx)) { best = b2; bidx = i2; }
    }
    if (lane == 0) { sm[wave] = m; ss[wave] = s; sx[wave] = sum; sb[wave] = best; si[wave] = bidx; }
    __syncthreads();
    const float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    float S = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) S += ss[w] * __expf(sm[w] - M);
    const float lse = M + __logf(S);
    if (tid == 0) {
        const float xt = bf2f(x[label]);
        float B = sb[0];
        int I = si[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (sb[w] > B || (sb[w] == B && si[w] < I)) { B = sb[w]; I = si[w]; }
        // sum_c q_c (log q_c - log p_c) = C + lse - (1 - eps) x_t - eps / (V - 1) sum_{c != t} x_c     (the q_c sum to 1)
        const float SX = (sx[0] + sx[1]) + (sx[2] + sx[3]);
        a.row_loss[row] = a.eps > 0.f ? (a.C + lse) - (1.f - a.eps) * xt - a.q_other * (SX - xt) : lse - xt;
        a.row_lse[row] = lse;
        a.correct[row] = I == (int)label ? 1 : 0;
        if (FUSED) a.kept[row] = 1;
    }
    if (!FUSED || !write_grad) return;
    __syncthreads();                                       // x[label] read before anybody overwrites it
    cap_grad_row(x, nchunk, V, label, lse, 1.f - a.eps, a.q_other, a.scale, tid);
}

// selection in the style of rank_kernel (retrieval.hip): a labelled row is kept when fewer than k labelled rows sort before it by
// (loss ascending, row ascending) -- torch.topk(largest=False) up to its order among equal losses; NaN sorts last.  Then the gradient pass.
__global__ __launch_bounds__(256) void cap_select_kernel(CapArgs a, int write_grad) {
    __shared__ int wred[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    bf16_t* x = a.logits + (long)row * a.ld;
    const long label = a.labels[row];
    const int nchunk = (int)(a.ld / 8);
    if (label < 0 || label >= a.V) {
        if (write_grad) cap_zero_row(x, nchunk, tid);
        return;
    }
    const float mine = a.row_loss[row];
    const bool mnan = isnan(mine);
    int cnt = 0;
    for (int r = tid; r < a.rows; r += 256) {
        const long lr = a.labels[r];
        if (lr < 0 || lr >= a.V) continue;
        const float l = a.row_loss[r];
        const bool lnan = isnan(l);
        const bool before = mnan ? (!lnan || r < row) : (!lnan && (l < mine || (l == mine && r < row)));
        cnt += before ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) wred[tid >> 6] = cnt;
    __syncthreads();
    const bool keep = (wred[0] + wred[1]) + (wred[2] + wred[3]) < a.k;
    if (tid == 0) a.kept[row] = keep ? 1 : 0;
    if (!write_grad) return;
    if (keep) cap_grad_row(x, nchunk, a.V, label, a.row_lse[row], 1.f - a.eps, a.q_other, a.scale, tid);
    else cap_zero_row(x, nchunk, tid);
}

// out = {sum of the kept row losses, k, number of correct rows, number of labelled rows}: one block, fixed order
__global__ __launch_bounds__(256) void cap_total_kernel(CapArgs a) {
    __shared__ float sl[4];
    __shared__ int sc[4], sn[4];
    const int tid = threadIdx.x;
    float ls = 0.f;
    int nc = 0, nl = 0;
    for (int r = tid; r < a.rows; r += 256) {
        const long lr = a.labels[r];
        if (lr < 0 || lr >= a.V) continue;
        ++nl;
        nc += a.correct[r];
        if (a.kept[r]) ls += a.row_loss[r];
    }
    ls = wave_sum(ls);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nc += __shfl_xor(nc, o, 64); nl += __shfl_xor(nl, o, 64); }
    if ((tid & 63) == 0) { sl[tid >> 6] = ls; sc[tid >> 6] = nc; sn[tid >> 6] = nl; }
    __syncthreads();
    if (tid == 0) {
        a.out[0] = (sl[0] + sl[1]) + (sl[2] + sl[3]);
        a.out[1] = (float)a.k;
        a.out[2] = (float)((sc[0] + sc[1]) + (sc[2] + sc[3]));
        a.out[3] = (float)((sn[0] + sn[1]) + (sn[2] + sn[3]));
    }
}

extern "C" int lav_caption_loss_fwd_bwd(void* stream, int rows, int V, void* logits, long ld, const int64_t* labels, float label_smoothing,
                                        int k, int select, float* row_loss, float* row_lse, int32_t* correct, int32_t* kept, float* out,
                                        int write_grad) {
    LAV_REQUIRE(rows > 0 && V > 1 && logits && labels && row_loss && row_lse && correct && kept && out, "lav_caption_loss_fwd_bwd: bad arguments");
    LAV_REQUIRE(ld % 8 == 0 && ld >= V, "lav_caption_loss_fwd_bwd: ld must be a multiple of 8 and >= V");
    LAV_REQUIRE(label_smoothing >= 0.f && label_smoothing < 1.f, "lav_caption_loss_fwd_bwd: label_smoothing %g outside [0, 1)", (double)label_smoothing);
    LAV_REQUIRE(k >= 0 && k <= rows, "lav_caption_loss_fwd_bwd: k = %d kept rows of %d", k, rows);
    CapArgs a;
    a.rows = rows; a.V = V; a.k = k; a.logits = (bf16_t*)logits; a.ld = ld; a.labels = labels;
    const double e = (double)label_smoothing;
    a.eps = label_smoothing;
    a.C = (float)((1.0 - e) * log(1.0 - e) + (e > 0.0 ? e * log(e / (double)(V - 1)) : 0.0));
    a.q_other = (float)(e / (double)(V - 1));
    a.scale = k > 0 ? 1.f / (float)k : 0.f;
    a.row_loss = row_loss; a.row_lse = row_lse; a.correct = correct; a.kept = kept; a.out = out;
    hipStream_t st = (hipStream_t)stream;
    if (select) {
        hipLaunchKernelGGL(cap_row_kernel<false>, dim3(rows), dim3(256), 0, st, a, 0);
        hipLaunchKernelGGL(cap_select_kernel, dim3(rows), dim3(256), 0, st, a, write_grad);
    } else {
        hipLaunchKernelGGL(cap_row_kernel<true>, dim3(rows), dim3(256), 0, st, a, write_grad);
    }
    hipLaunchKernelGGL(cap_total_kernel, dim3(1), dim3(256), 0, st, a);
    return lav_check_launch("lav_caption_loss_fwd_bwd");
}

__global__ __launch_bounds__(256) void scale_bf16_kernel(long n8, bf16_t* x, const float* cnt, float gscale) {
    const float s = cnt ? gscale / fmaxf(cnt[1], 1.f) : gscale;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        float v[8];
        uint4 u = *(uint4*)(x + i * 8);
        unpack8(u, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] *= s;
        *(uint4*)(x + i * 8) = pack8(v);
    }
}

// x *= scalar[0] with the scalar read ON THE DEVICE (an upstream autograd gradient): no host round trip; a scalar of
// exactly 1 (loss = ls_mtm + ls_vtm, main_pretrain_mlm.py:163) leaves after one load per thread
template <bool F32>
__global__ __launch_bounds__(256) void scale_scalar_kernel(long n8, void* x, const float* scalar) {
    const float s = scalar[0];
    if (s == 1.f) return;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        if (F32) {
            float4* p = (float4*)x + 2 * i;
            float4 a = p[0], b = p[1];
            a.x *= s; a.y *= s; a.z *= s; a.w *= s; b.x *= s; b.y *= s; b.z *= s; b.w *= s;
            p[0] = a; p[1] = b;
        } else {
            float v[8];
            uint4 u = *((uint4*)x + i);
            unpack8(u, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] *= s;
            *((uint4*)x + i) = pack8(v);
        }
    }
}

extern "C" int lav_scale_by_scalar(void* stream, long n_elems, void* x, int x_is_f32, const float* scalar_dev) {
    LAV_REQUIRE(n_elems > 0 && n_elems % 8 == 0 && x && scalar_dev, "lav_scale_by_scalar: bad arguments (n must be a multiple of 8)");
    long n8 = n_elems / 8;
    int grid = (int)((n8 + 255) / 256 > 8192 ? 8192 : (n8 + 255) / 256);
    if (x_is_f32) hipLaunchKernelGGL(scale_scalar_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, n8, x, scalar_dev);
    else hipLaunchKernelGGL(scale_scalar_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, n8, x, scalar_dev);
    return lav_check_launch("lav_scale_by_scalar");
}

extern "C" int lav_scale_by_count(void* stream, long n_elems, void* x_bf16, const float* loss_sum, float gscale) {
    LAV_REQUIRE(n_elems > 0 && n_elems % 8 == 0 && x_bf16, "lav_scale_by_count: bad arguments");
    long n8 = n_elems / 8;
    int grid = (int)((n8 + 255) / 256 > 8192 ? 8192 : (n8 + 255) / 256);
    hipLaunchKernelGGL(scale_bf16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n8, (bf16_t*)x_bf16, loss_sum, gscale);
    return lav_check_launch("lav_scale_by_count");
}

// ---- video-text matching score head (main_pretrain_task_specific.py:128-133,168-170) ------------------
// last layer of self.fc = Linear(2H, 1): one score per (video, text) pair, divided by the temperature and laid
// out as the (B, O) logit matrix the cross-entropy consumes.  One wave per pair row.
__global__ __launch_bounds__(256) void pair_score_fwd_kernel(int n, int F, const bf16_t* __restrict__ h, long ldh,
                                                            const bf16_t* __restrict__ w, const float* __restrict__ b,
                                                            float inv_temp, int O, float* __restrict__ logits, long ld) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const bf16_t* x = h + (long)row * ldh;
    float s = 0.f;
    for (int c = lane; c < F / 8; c += 64) {
        float a[8], ww[8];
        unpack8(*(const uint4*)(x + c * 8), a);
        unpack8(*(const uint4*)(w + c * 8), ww);
#pragma unroll
        for (int k = 0; k < 8; ++k) s += a[k] * ww[k];
    }
    s = wave_sum(s);
    if (lane == 0) logits[(long)(row / O) * ld + row % O] = (s + b[0]) * inv_temp;
}

// backward of the score head: dz = dlogits * inv_temp; dh = dz * w * act'(z1) (act' stored by the first GEMM);
// dw += sum_r dz_r h_r; db += sum_r dz_r.  One block per 32 pair rows, thread t owns columns 8t..8t+7.
__global__ __launch_bounds__(256) void pair_score_bwd_kernel(int n, int F, const float* __restrict__ dlogits, long ld, int O,
                                                            float inv_temp, const bf16_t* __restrict__ h, long ldh,
                                                            const bf16_t* __restrict__ act_grad, long ldg,
                                                            const bf16_t* __restrict__ w, bf16_t* __restrict__ dh, long lddh,
                                                            float* __restrict__ dw, float* __restrict__ db) {
    const int r0 = blockIdx.x * 32, r1 = min(n, r0 + 32);
    float dbs = 0.f;
    for (int c = threadIdx.x; c < F / 8; c += 256) {
        float ww[8], acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        unpack8(*(const uint4*)(w + c * 8), ww);
        for (int r = r0; r < r1; ++r) {
            const float dz = dlogits[(long)(r / O) * ld + r % O] * inv_temp;
            float a[8], g[8], o[8];
            unpack8(*(const uint4*)(h + (long)r * ldh + c * 8), a);
            if (act_grad) unpack8(*(const uint4*)(act_grad + (long)r * ldg + c * 8), g);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                acc[k] += dz * a[k];
                o[k] = dz * ww[k] * (act_grad ? g[k] : 1.f);
            }
            *(uint4*)(dh + (long)r * lddh + c * 8) = pack8(o);
            if (c == 0) dbs += dz;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) atomicAdd(dw + c * 8 + k, acc[k]);
    }
    if (threadIdx.x == 0) atomicAdd(db, dbs);
}

extern "C" int lav_pair_score_fwd(void* stream, int n, int F, const void* h, long ldh, const void* w_bf16, const float* bias,
                                  float inv_temp, int O, void* logits, long ld) {
    LAV_REQUIRE(n > 0 && F > 0 && F % 8 == 0 && O > 0 && n % O == 0 && ld >= O && ldh % 8 == 0 && h && w_bf16 && bias && logits,
                "lav_pair_score_fwd: bad arguments");
    hipLaunchKernelGGL(pair_score_fwd_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, n, F, (const bf16_t*)h, ldh,
                       (const bf16_t*)w_bf16, bias, inv_temp, O, (float*)logits, ld);
    return lav_check_launch("lav_pair_score_fwd");
}

extern "C" int lav_pair_score_bwd(void* stream, int n, int F, const void* dlogits, long ld, int O, float inv_temp, const void* h,
                                  long ldh, const void* act_grad, long ldg, const void* w_bf16, void* dh, long lddh, float* dw,
                                  float* db) {
    LAV_REQUIRE(n > 0 && F > 0 && F % 8 == 0 && O > 0 && n % O == 0 && ld >= O && ldh % 8 == 0 && lddh % 8 == 0 &&
                (!act_grad || ldg % 8 == 0) && dlogits && h && w_bf16 && dh && dw && db, "lav_pair_score_bwd: bad arguments");
    hipLaunchKernelGGL(pair_score_bwd_kernel, dim3((n + 31) / 32), dim3(256), 0, (hipStream_t)stream, n, F, (const float*)dlogits, ld,
                       O, inv_temp, (const bf16_t*)h, ldh, (const bf16_t*)act_grad, ldg, (const bf16_t*)w_bf16, (bf16_t*)dh, lddh, dw, db);
    return lav_check_launch("lav_pair_score_bwd");
}

// ---- optimizer over the flat arena ------------------------------------------------------------------
// sum of squares, DETERMINISTIC (fixed grid, fixed reduction order): the clip coefficient derived from it must be
// bit-identical on every data-parallel rank, otherwise the replicas drift apart by ulps per step.
#define SUMSQ_BLOCKS 1024
__device__ float g_sumsq_partial[SUMSQ_BLOCKS];

__global__ __launch_bounds__(256) void sumsq_kernel(long n, const float* g) {
    float s = 0.f;
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)SUMSQ_BLOCKS * 256) {
        float4 v = ((const float4*)g)[i];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long i = n4 * 4; i < n; ++i) s += g[i] * g[i];
    s = wave_sum(s);
    __shared__ float sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) g_sumsq_partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void sumsq_final_kernel(float* out) {
    float s = 0.f;
    for (int i = threadIdx.x; i < SUMSQ_BLOCKS; i += 256) s += g_sumsq_partial[i];
    s = wave_sum(s);
    __shared__ float sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] += (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

extern "C" int lav_sumsq_f32(void* stream, long n, const float* g, float* out) {
    LAV_REQUIRE(n > 0 && g && out && ((uintptr_t)g % 16) == 0, "lav_sumsq_f32: bad arguments");
    hipLaunchKernelGGL(sumsq_kernel, dim3(SUMSQ_BLOCKS), dim3(256), 0, (hipStream_t)stream, n, g);
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, out);
    return lav_check_launch("lav_sumsq_f32");
}

struct AdamArgs {
    long n; float* p; const float* g; float* m; float* v; bf16_t* pb;
    const uint8_t* grp;
    float lr[4], wd[4];
    float b1, b2, eps, bc1, bc2, max_norm, grad_div;
    const float* gradsq;
    int nt;
};

__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a) {
    float coef = 1.f / a.grad_div;
    if (a.gradsq && a.max_norm > 0.f) {
        // clip_grad_norm_ (agent.py:246): total norm of the (already averaged) gradient
        const float tn = sqrtf(a.gradsq[0]) / a.grad_div;
        const float c = a.max_norm / (tn + 1e-6f);
        if (c < 1.f) coef *= c;
    }
    const long n4 = a.n / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 p = ((float4*)a.p)[i], g = ((const float4*)a.g)[i], m = ((float4*)a.m)[i], v = ((float4*)a.v)[i];
        float pp[4] = {p.x, p.y, p.z, p.w}, gg[4] = {g.x, g.y, g.z, g.w}, mm[4] = {m.x, m.y, m.z, m.w}, vv[4] = {v.x, v.y, v.z, v.w};
        const int gv = a.grp ? a.grp[i >> 4] : 0;
        // bit 2: a parameter that never receives a gradient on this path (emb_task, enc_img.emb_odr).  In the reference its
        // .grad is None and torch.optim.AdamW skips the tensor entirely -- no weight decay, no moment update
        if (gv & 4) continue;
        const int gi = gv & 3;
        const float lr = a.lr[gi], wd = a.wd[gi];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gk = gg[k] * coef;
            pp[k] *= 1.f - lr * wd;
            mm[k] = a.b1 * mm[k] + (1.f - a.b1) * gk;
            vv[k] = a.b2 * vv[k] + (1.f - a.b2) * gk * gk;
            const float denom = sqrtf(vv[k]) / sqrtf(a.bc2) + a.eps;
            pp[k] -= (lr / a.bc1) * mm[k] / denom;
        }
        if (a.nt) {                                       // LAV_NT_STORES & 2 (off by default: measured neutral, 75.1 vs 75.0 ms per step)
            typedef float lav_f32x4 __attribute__((ext_vector_type(4)));
            const lav_f32x4 pv = {pp[0], pp[1], pp[2], pp[3]}, mv = {mm[0], mm[1], mm[2], mm[3]}, vv4 = {vv[0], vv[1], vv[2], vv[3]};
            __builtin_nontemporal_store(pv, (lav_f32x4*)a.p + i);
            __builtin_nontemporal_store(mv, (lav_f32x4*)a.m + i);
            __builtin_nontemporal_store(vv4, (lav_f32x4*)a.v + i);
        } else {
            ((float4*)a.p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
            ((float4*)a.m)[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
            ((float4*)a.v)[i] = make_float4(vv[0], vv[1], vv[2], vv[3]);
        }
        if (a.pb) {
            uint2 w; w.x = pack2(pp[0], pp[1]); w.y = pack2(pp[2], pp[3]);
            ((uint2*)a.pb)[i] = w;
        }
    }
}

extern "C" int lav_adamw_step(void* stream, long n, float* p, const float* g, float* m, float* v, void* p_bf16,
                              const uint8_t* block_group, const float lr[4], const float wd[4], float beta1, float beta2,
                              float eps, int step, const float* gradsq, float max_norm, float grad_div) {
    LAV_REQUIRE(n > 0 && n % 64 == 0 && p && g && m && v && lr && wd, "lav_adamw_step: n must be a positive multiple of 64 (arena blocks)");
    LAV_REQUIRE(step >= 1, "lav_adamw_step: step counts from 1");
    AdamArgs a;
    a.n = n; a.p = p; a.g = g; a.m = m; a.v = v; a.pb = (bf16_t*)p_bf16;
    a.grp = block_group;
    static const int nt_stores = getenv("LAV_NT_STORES") ? atoi(getenv("LAV_NT_STORES")) : 1;
    a.nt = (nt_stores >> 1) & 1;
    for (int k = 0; k < 4; ++k) { a.lr[k] = lr[k]; a.wd[k] = wd[k]; }
    a.b1 = beta1; a.b2 = beta2; a.eps = eps;
    a.bc1 = 1.f - powf(beta1, (float)step); a.bc2 = 1.f - powf(beta2, (float)step);
    a.max_norm = max_norm; a.grad_div = grad_div > 0.f ? grad_div : 1.f; a.gradsq = gradsq;
    int grid = (int)((n / 4 + 255) / 256 > 4096 ? 4096 : (n / 4 + 255) / 256);
    hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    return lav_check_launch("lav_adamw_step");
}

__global__ __launch_bounds__(256) void cast_kernel(long n, const float* in, bf16_t* out) {
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 v = ((const float4*)in)[i];
        uint2 w; w.x = pack2(v.x, v.y); w.y = pack2(v.z, v.w);
        ((uint2*)out)[i] = w;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long i = n4 * 4; i < n; ++i) out[i] = f2bf(in[i]);
}

// bf16 -> fp32 (the summed half-precision gradient buckets of the data-parallel exchange back into the fp32 gradient arena)
__global__ __launch_bounds__(256) void widen_kernel(long n, const bf16_t* __restrict__ in, float* __restrict__ out) {
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += (long)gridDim.x * 256 * 8) {
        if (i + 8 <= n) {
            float f[8];
            unpack8(*(const uint4*)(in + i), f);
            *(float4*)(out + i) = *(const float4*)&f[0]; *(float4*)(out + i + 4) = *(const float4*)&f[4];
        } else {
            for (long k = i; k < n; ++k) out[k] = bf2f(in[k]);
        }
    }
}

extern "C" int lav_cast_bf16_to_f32(void* stream, long n, const void* in, float* out) {
    LAV_REQUIRE(n > 0 && in && out && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0, "lav_cast_bf16_to_f32: bad arguments (16-byte aligned buffers)");
    int grid = (int)((n / 8 + 255) / 256 > 4096 ? 4096 : (n / 8 + 255) / 256);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(widen_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, (const bf16_t*)in, out);
    return lav_check_launch("lav_cast_bf16_to_f32");
}

extern "C" int lav_cast_f32_to_bf16(void* stream, long n, const float* in, void* out) {
    LAV_REQUIRE(n > 0 && in && out, "lav_cast_f32_to_bf16: bad arguments");
    int grid = (int)((n / 4 + 255) / 256 > 4096 ? 4096 : (n / 4 + 255) / 256);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(cast_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, in, (bf16_t*)out);
    return lav_check_launch("lav_cast_f32_to_bf16");
}

// ---- batched bf16 transpose of the weight matrices (second working copy of the parameter arena) ---------------------
// dX = dY . W contracts over the ROWS of W (out-features): with only W in memory the matrix cores need transposing LDS
// reads for that operand (ds_read_b64_tr_b16), measured 20-25 % slower than the K-contiguous path.  Keeping W^T next to
// W turns every input-gradient GEMM into the forward layout; the copy is refreshed once per optimizer step (one launch
// over all matrices, 443 MB read + written).
__global__ __launch_bounds__(256) void transpose_batched_kernel(int n_mats, const lav_mat_desc* __restrict__ descs, const bf16_t* __restrict__ src,
                                                               bf16_t* __restrict__ dst) {
    __shared__ uint16_t tile[64][66];
    int lo = 0, hi = n_mats - 1;                          // last matrix whose first tile is <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].tile0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const lav_mat_desc d = descs[lo];
    const int t = blockIdx.x - d.tile0, tiles_c = (d.cols + 63) / 64;
    const int r0 = (t / tiles_c) * 64, c0 = (t % tiles_c) * 64;
    const uint16_t* S = (const uint16_t*)src + d.src_off;
    uint16_t* D = (uint16_t*)dst + d.dst_off;
    for (int i = threadIdx.x; i < 512; i += 256) {        // 64 rows x 8 chunks of 8 columns
        const int r = i >> 3, ch = i & 7, gr = r0 + r, gc = c0 + ch * 8;
        uint16_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (gr < d.rows) {
            if (gc + 8 <= d.cols) *(uint4*)v = *(const uint4*)(S + (long)gr * d.cols + gc);
            else for (int k = 0; k < 8; ++k) if (gc + k < d.cols) v[k] = S[(long)gr * d.cols + gc + k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[r][ch * 8 + k] = v[k];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += 256) {        // 64 output rows (source columns) x 8 chunks of 8 source rows
        const int c = i >> 3, ch = i & 7, gc = c0 + c, gr = r0 + ch * 8;
        if (gc >= d.cols || gr >= d.rows) continue;
        uint16_t v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = tile[ch * 8 + k][c];
        uint16_t* o = D + (long)gc * d.ld_dst + gr;
        if (gr + 8 <= d.rows) *(uint4*)o = *(const uint4*)v;
        else for (int k = 0; k < 8; ++k) if (gr + k < d.rows) o[k] = v[k];
    }
}

extern "C" int lav_transpose_bf16_batched(void* stream, int n_mats, const lav_mat_desc* descs_dev, int total_tiles, const void* src,
                                          void* dst) {
    LAV_REQUIRE(n_mats > 0 && total_tiles > 0 && descs_dev && src && dst, "lav_transpose_bf16_batched: bad arguments");
    hipLaunchKernelGGL(transpose_batched_kernel, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, n_mats, descs_dev, (const bf16_t*)src,
                       (bf16_t*)dst);
    return lav_check_launch("lav_transpose_bf16_batched");
}

// per-sample stochastic depth factors (video_swin.py:46-54): scale = floor(keep + u) / keep
__global__ void droppath_kernel(int n_blocks, int B, const float* keep_prob, uint32_t seed, float* scale) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_blocks * B) return;
    const float keep = keep_prob[i / B];
    const float u = (float)(lav_mix(lav_mix((uint32_t)i * 0x9E3779B9u + seed)) >> 8) * (1.0f / 16777216.0f);
    scale[i] = keep >= 1.f ? 1.f : floorf(keep + u) / keep;
}

extern "C" int lav_fill_droppath(void* stream, int n_blocks, int B, const float* keep_prob, uint32_t seed, float* scale) {
    LAV_REQUIRE(n_blocks > 0 && B > 0 && keep_prob && scale, "lav_fill_droppath: bad arguments");
    int n = n_blocks * B;
    hipLaunchKernelGGL(droppath_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_blocks, B, keep_prob, seed, scale);
    return lav_check_launch("lav_fill_droppath");
}

// ---- zero a list of 64-element blocks of the gradient arena (the parts that are NOT first-touch weight gradients: vectors and tables written with
// atomics): one launch instead of an 886 MB fill -- 16 threads per block, 16 bytes each -------------------------------------------------------
__global__ __launch_bounds__(256) void zero_blocks_kernel(float* __restrict__ base, const int32_t* __restrict__ blocks, long n_blocks, int block_elems) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int per = block_elems >> 2;                          // float4 stores per block
    const long b = t / per;
    if (b >= n_blocks) return;
    *(float4*)(base + (long)blocks[b] * block_elems + (t - b * per) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
}

extern "C" int lav_zero_blocks(void* stream, float* base, const int32_t* blocks, long n_blocks, int block_elems) {
    LAV_REQUIRE(base && (n_blocks == 0 || blocks) && n_blocks >= 0 && block_elems >= 4 && block_elems % 4 == 0 && ((uintptr_t)base & 15) == 0,
                "lav_zero_blocks: bad arguments (n_blocks %ld, block_elems %d)", n_blocks, block_elems);
    if (n_blocks == 0) return LAV_OK;
    const long threads = n_blocks * (block_elems >> 2);
    hipLaunchKernelGGL(zero_blocks_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, base, blocks, n_blocks, block_elems);
    return lav_check_launch("lav_zero_blocks");
}
