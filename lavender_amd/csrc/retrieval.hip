// Text-to-video retrieval evaluation kernels (eval only): the parts of eval_retrieval_mlm.py:138-247 that the (caption, video) pair
// scorer needs beyond the fusion layers.  Only the appended [MASK] row of each pair reaches the score, so:
//   attn_rows       one selected query row per sequence against all L keys of that sequence, per head (head_dim 64), fp32 softmax.
//                   One workgroup per (sequence, head); 8 lanes share one 128-byte key / value row.  No MFMA: one query row is a
//                   matrix-vector product, bound by the key / value reads.
//   pair_readout    the rest of BertOnlyMLMHead on those rows after the transform GEMM: fp32 LayerNorm, the two decoder rows of the
//                   "true" / "false" tokens + the tied bias, s = p_true / (p_true + p_false) (eval_retrieval_mlm.py:203-206) stored
//                   into a caller-owned score matrix.  One wave per row.
//   rank            rank of the ground-truth column in each row of the score matrix (the stable sort of :223-227).
// No atomics and fixed reduction orders everywhere: two runs give identical bits.
#include "common.h"
#include <math.h>
#include <string.h>
#include "../../include/lavender_hip.h"

#define AR_THREADS 256
#define AR_GROUPS (AR_THREADS / 8)                 // key rows in flight per pass: 8 lanes x 16 bytes = one 64-wide bf16 head row
#define AR_MAX_L 4096

__global__ __launch_bounds__(AR_THREADS) void attn_rows_kernel(int L, int heads, const bf16_t* __restrict__ qkv, long ldq,
                                                              const int32_t* __restrict__ key_mask, const int32_t* __restrict__ q_row,
                                                              float scale, bf16_t* __restrict__ out, long ldo) {
    __shared__ float sc[AR_MAX_L];
    __shared__ float red[AR_GROUPS][64 + 1];
    __shared__ float wred[AR_THREADS / 64];
    const int s = blockIdx.x / heads, h = blockIdx.x % heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = tid >> 3, c = tid & 7;         // key row handled by this lane group, 16-byte chunk of the head row
    const int H = heads * 64;
    const int qr = q_row[s];
    bf16_t* o = out + (long)s * ldo + h * 64;
    if (qr < 0 || qr >= L) {                       // no valid query row: the output row is zero (nothing is read)
        if (tid < 64) o[tid] = 0;
        return;
    }
    const bf16_t* base = qkv + (long)s * L * ldq;
    float q[8];
    unpack8(*(const uint4*)(base + (long)qr * ldq + h * 64 + c * 8), q);
    const int32_t* km = key_mask + (long)s * L;
    // scores of every key
    for (int j = grp; j < L; j += AR_GROUPS) {
        float k[8];
        unpack8(*(const uint4*)(base + (long)j * ldq + H + h * 64 + c * 8), k);
        float d = 0.f;
#pragma unroll
        for (int x = 0; x < 8; ++x) d = fmaf(q[x], k[x], d);
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);
        d += __shfl_xor(d, 4, 64);
        if (c == 0) sc[j] = km[j] ? d * scale : -INFINITY;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = tid; j < L; j += AR_THREADS) m = fmaxf(m, sc[j]);
    m = wave_max(m);
    if (lane == 0) wred[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
    __syncthreads();
    float l = 0.f;
    for (int j = tid; j < L; j += AR_THREADS) {
        const float p = (m == -INFINITY || sc[j] == -INFINITY) ? 0.f : expf(sc[j] - m);
        sc[j] = p;
        l += p;
    }
    l = wave_sum(l);
    if (lane == 0) wred[wave] = l;
    __syncthreads();
    l = (wred[0] + wred[1]) + (wred[2] + wred[3]);
    // p . V: lane group grp sums the keys grp, grp + 32, ... for its 8 columns; the 32 partials meet in LDS in a fixed order
    float acc[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) acc[x] = 0.f;
    for (int j = grp; j < L; j += AR_GROUPS) {
        const float p = sc[j];
        if (p == 0.f) continue;
        float v[8];
        unpack8(*(const uint4*)(base + (long)j * ldq + 2 * H + h * 64 + c * 8), v);
#pragma unroll
        for (int x = 0; x < 8; ++x) acc[x] = fmaf(p, v[x], acc[x]);
    }
#pragma unroll
    for (int x = 0; x < 8; ++x) red[grp][c * 8 + x] = acc[x];
    __syncthreads();
    if (tid < 64) {
        float t = 0.f;
        for (int g = 0; g < AR_GROUPS; ++g) t += red[g][tid];
        o[tid] = f2bf(l > 0.f ? t / l : 0.f);
    }
}

extern "C" int lav_attention_rows(void* stream, int n, int L, int heads, int head_dim, const void* qkv, long ldq, const int32_t* key_mask,
                                  const int32_t* q_row, float scale, void* out, long ldo) {
    LAV_REQUIRE(n > 0 && L > 0 && L <= AR_MAX_L && heads > 0 && head_dim == 64, "lav_attention_rows: n=%d L=%d (1..%d) heads=%d head_dim=%d (64)",
                n, L, AR_MAX_L, heads, head_dim);
    LAV_REQUIRE(qkv && key_mask && q_row && out, "lav_attention_rows: null pointer");
    LAV_REQUIRE(((uintptr_t)qkv & 15) == 0, "lav_attention_rows: qkv must be 16-byte aligned (its rows are read in 16-byte chunks)");
    LAV_REQUIRE(ldq >= 3L * heads * 64 && (ldq % 8) == 0 && ldo >= (long)heads * 64 && (ldo % 8) == 0,
                "lav_attention_rows: ldq=%ld (>= 3 hidden, multiple of 8) ldo=%ld (>= hidden, multiple of 8)", ldq, ldo);
    hipLaunchKernelGGL(attn_rows_kernel, dim3((unsigned)n * heads), dim3(AR_THREADS), 0, (hipStream_t)stream, L, heads, (const bf16_t*)qkv, ldq,
                       key_mask, q_row, scale, (bf16_t*)out, ldo);
    return lav_check_launch("lav_attention_rows");
}

#define PR_THREADS 256
#define PR_MAX_PER_LANE 16                         // hidden <= 1024

__global__ __launch_bounds__(PR_THREADS) void pair_readout_kernel(int n, int H, const float* __restrict__ t, long ldt, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps, const bf16_t* __restrict__ w_true,
                                                                 const bf16_t* __restrict__ w_false, const float* __restrict__ b_dec, int true_id, int false_id,
                                                                 const int32_t* __restrict__ orow, const int32_t* __restrict__ ocol,
                                                                 float* __restrict__ S, long ldS, int s_rows, int s_cols, float* __restrict__ logits) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (PR_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= n) return;
    const float* tr = t + (long)r * ldt;
    float v[PR_MAX_PER_LANE];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < PR_MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < H ? tr[c] : 0.f;
        sum += v[i];
    }
    const float mean = wave_sum(sum) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PR_MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        const float d = c < H ? v[i] - mean : 0.f;
        q = fmaf(d, d, q);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + eps);
    float pt = 0.f, pf = 0.f;
#pragma unroll
    for (int i = 0; i < PR_MAX_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        if (c < H) {
            const float xn = (v[i] - mean) * rstd * gamma[c] + beta[c];
            pt = fmaf(xn, bf2f(w_true[c]), pt);
            pf = fmaf(xn, bf2f(w_false[c]), pf);
        }
    }
    pt = wave_sum(pt) + b_dec[true_id];
    pf = wave_sum(pf) + b_dec[false_id];
    if (lane == 0) {
        const int rr = orow[r], cc = ocol[r];
        if (rr >= 0 && rr < s_rows && cc >= 0 && cc < s_cols) S[(long)rr * ldS + cc] = pt / (pt + pf);
        if (logits) { logits[2L * r] = pt; logits[2L * r + 1] = pf; }
    }
}

extern "C" int lav_mlm_pair_readout(void* stream, const lav_mlm_pair_readout_desc* d) {
    LAV_REQUIRE(d, "lav_mlm_pair_readout: null descriptor");
    LAV_REQUIRE(d->n > 0 && d->hidden > 0 && d->hidden % 64 == 0 && d->hidden <= 64 * PR_MAX_PER_LANE && d->vocab > 0,
                "lav_mlm_pair_readout: n=%d hidden=%d (multiple of 64, <= %d) vocab=%d", d->n, d->hidden, 64 * PR_MAX_PER_LANE, d->vocab);
    LAV_REQUIRE(d->true_id >= 0 && d->true_id < d->vocab && d->false_id >= 0 && d->false_id < d->vocab,
                "lav_mlm_pair_readout: true_id=%d false_id=%d outside the vocabulary (%d)", d->true_id, d->false_id, d->vocab);
    LAV_REQUIRE(d->x && d->w_dense && d->b_dense && d->ln_gamma && d->ln_beta && d->w_dec && d->b_dec && d->t && d->out_row && d->out_col && d->scores,
                "lav_mlm_pair_readout: null pointer");
    LAV_REQUIRE(d->score_rows > 0 && d->score_cols > 0 && d->ld_scores >= d->score_cols && d->ldw_dec >= d->hidden && d->ldx >= d->hidden,
                "lav_mlm_pair_readout: scores %d x %d (ld %ld), ldw_dec %ld, ldx %ld", d->score_rows, d->score_cols, d->ld_scores, d->ldw_dec, d->ldx);
    const int n = d->n, H = d->hidden;
    // t = gelu(x Wt^T + b), fp32: the transform dense of BertPredictionHeadTransform on the tile GEMM
    {
        lav_gemm_epilogue e;
        memset(&e, 0, sizeof(e));
        e.alpha = 1.f; e.rows_per_group = 1; e.k_rows_per_group = 1; e.bias = d->b_dense; e.act = 1; e.out_mode = 1;
        const int rc = lav_gemm_bf16(stream, 0, n, H, H, d->x, d->ldx, d->w_dense, H, d->t, H, &e, 1);
        if (rc != LAV_OK) return rc;
    }
    const bf16_t* w = (const bf16_t*)d->w_dec;
    hipLaunchKernelGGL(pair_readout_kernel, dim3((n + PR_THREADS / 64 - 1) / (PR_THREADS / 64)), dim3(PR_THREADS), 0, (hipStream_t)stream, n, H,
                       d->t, (long)H, d->ln_gamma, d->ln_beta, d->ln_eps, w + (long)d->true_id * d->ldw_dec, w + (long)d->false_id * d->ldw_dec,
                       d->b_dec, d->true_id, d->false_id, d->out_row, d->out_col, d->scores, d->ld_scores, d->score_rows, d->score_cols, d->logits);
    return lav_check_launch("lav_mlm_pair_readout");
}

// rank of column gt[t] in row t: 1 + #{v : v sorts before gt}, the order of a stable sort by -score over the columns in their order
// (eval_retrieval_mlm.py:223-227).  NaN sorts after every number, NaNs among themselves by column.
#define RK_THREADS 256

__global__ __launch_bounds__(RK_THREADS) void rank_kernel(int M, const float* __restrict__ S, long ldS, const int32_t* __restrict__ gt, int32_t* __restrict__ out) {
    __shared__ int wred[RK_THREADS / 64];
    const int t = blockIdx.x, tid = threadIdx.x;
    const int g = gt[t];
    if (g < 0 || g >= M) {                         // no ground-truth column: rank 0 marks the row
        if (tid == 0) out[t] = 0;
        return;
    }
    const float* row = S + (long)t * ldS;
    const float sg = row[g];
    const bool gnan = isnan(sg);
    int cnt = 0;
    for (int v = tid; v < M; v += RK_THREADS) {
        const float x = row[v];
        const bool xnan = isnan(x);
        const bool before = gnan ? (!xnan || v < g) : (!xnan && (x > sg || (x == sg && v < g)));
        cnt += before ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) wred[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) out[t] = 1 + (wred[0] + wred[1]) + (wred[2] + wred[3]);
}

extern "C" int lav_retrieval_rank(void* stream, int n_text, int n_video, const float* S, long ldS, const int32_t* gt, int32_t* out) {
    LAV_REQUIRE(n_text > 0 && n_video > 0 && ldS >= n_video, "lav_retrieval_rank: n_text=%d n_video=%d ldS=%ld", n_text, n_video, ldS);
    LAV_REQUIRE(S && gt && out, "lav_retrieval_rank: null pointer");
    hipLaunchKernelGGL(rank_kernel, dim3(n_text), dim3(RK_THREADS), 0, (hipStream_t)stream, n_video, S, ldS, gt, out);
    return lav_check_launch("lav_retrieval_rank");
}
