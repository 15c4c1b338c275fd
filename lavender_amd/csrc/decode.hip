// Caption decoding kernels (eval only): the per-token work of LAVENDER_Captioning.generate with a key / value cache.
// Reference: model_for_captioning.py:139-500 (generate / _generate_no_beam_search, greedy and sampled) as driven by
// main_caption.py:98-125.  Each generated token sends 2 rows per clip through the fusion layers and B rows through the MLM head,
// shapes the tile GEMM (128-256-row tiles) and the sequence-attention kernels are not built for:
//   skinny_gemm      out[M, N] = x[M, K] . W[N, K]^T for M <= 64.  The weight is streamed once, straight to VGPRs as MFMA B
//                    fragments (no LDS staging: each fragment is used by this wave only); the x rows (a few KB) come from L2.
//                    One workgroup = 16 output columns, its four waves split K and meet in LDS (fixed order: deterministic).
//   attn_decode      q_len <= 8 new query rows per (clip, head) against [video keys (in place, by mask) ; cached text keys ;
//                    the new rows' own keys (causal)], fp32 softmax.  Keys are split over workgroups when B * heads is below the
//                    CU count; a second launch combines the partial (max, sum, output) triples in split order.
//   embed_rows       BERT embeddings of single rows with explicit positions.
//   greedy_step      repetition penalty, argmax (lowest index on a tie), log-softmax score, finished-row bookkeeping.
// No atomics anywhere: two runs give identical bits.
#include "common.h"
#include <math.h>
#include "../../include/lavender_hip.h"

#define SK_THREADS 256
#define SK_COLS 16

struct SkinnyArgs {
    const bf16_t* x; long ldx;
    const bf16_t* w; long ldw;
    int M, N, K;
    const float* bias;
    int epi;
    const void* res; long ldr; int res_bf16;
    void* out; long ldo;
};

__device__ __forceinline__ bf16x8 ld_frag(const bf16_t* p) { return *(const bf16x8*)p; }

template <int MT>
__global__ __launch_bounds__(SK_THREADS) void skinny_gemm_kernel(SkinnyArgs a) {
    __shared__ float red[4][MT * 16][SK_COLS + 1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n0 = blockIdx.x * SK_COLS;
    const int nk = a.K / 32;
    // B fragment: W row n0 + (lane & 15) (clamped: rows past N are read from row N - 1 and their results dropped), k slot lane >> 4
    const int nrow = min(n0 + (lane & 15), a.N - 1);
    const bf16_t* wp = a.w + (long)nrow * a.ldw + (lane >> 4) * 8;
    const bf16_t* xp[MT];
    bool xv[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = i * 16 + (lane & 15);
        xv[i] = m < a.M;
        xp[i] = a.x + (long)(xv[i] ? m : 0) * a.ldx + (lane >> 4) * 8;
    }
    f32x4 acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bf16x8 zero = {};
    // k-steps wave, wave + 4, ...: four steps in flight per wave (loads first, then the MFMAs)
    int ks = wave;
    for (; ks + 12 < nk; ks += 16) {
        bf16x8 b[4], x[4][MT];
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = ld_frag(wp + (ks + 4 * u) * 32);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < MT; ++i) x[u][i] = xv[i] ? ld_frag(xp[i] + (ks + 4 * u) * 32) : zero;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[u][i], b[u], acc[i], 0, 0, 0);
    }
    for (; ks < nk; ks += 4) {
        const bf16x8 b = ld_frag(wp + ks * 32);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const bf16x8 x = xv[i] ? ld_frag(xp[i] + ks * 32) : zero;
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, b, acc[i], 0, 0, 0);
        }
    }
    // accumulator: row (lane >> 4) * 4 + r of the 16-row block, column lane & 15
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][i * 16 + (lane >> 4) * 4 + r][lane & 15] = acc[i][r];
    __syncthreads();
    for (int idx = tid; idx < MT * 16 * SK_COLS; idx += SK_THREADS) {
        const int m = idx / SK_COLS, c = idx % SK_COLS, n = n0 + c;
        if (m >= a.M || n >= a.N) continue;
        float v = ((red[0][m][c] + red[1][m][c]) + red[2][m][c]) + red[3][m][c];
        if (a.bias) v += a.bias[n];
        switch (a.epi) {
            case LAV_SKINNY_BF16: ((bf16_t*)a.out)[(long)m * a.ldo + n] = f2bf(v); break;
            case LAV_SKINNY_GELU: ((bf16_t*)a.out)[(long)m * a.ldo + n] = f2bf(gelu_f(v)); break;
            case LAV_SKINNY_RES_F32: {
                const float r = a.res_bf16 ? bf2f(((const bf16_t*)a.res)[(long)m * a.ldr + n]) : ((const float*)a.res)[(long)m * a.ldr + n];
                ((float*)a.out)[(long)m * a.ldo + n] = v + r;
                break;
            }
            default: ((float*)a.out)[(long)m * a.ldo + n] = v; break;
        }
    }
}

extern "C" int lav_gemm_skinny_bf16(void* stream, int M, int N, int K, const void* x, long ldx, const void* w, long ldw,
                                    const float* bias, int epi, const void* residual, long ldr, int residual_bf16, void* out, long ldo) {
    LAV_REQUIRE(M >= 1 && M <= 64 && N >= 1 && K >= 32 && K % 32 == 0, "lav_gemm_skinny_bf16: M=%d (1..64) N=%d K=%d (multiple of 32)", M, N, K);
    LAV_REQUIRE(x && w && out, "lav_gemm_skinny_bf16: null pointer");
    LAV_REQUIRE(ldx >= K && ldw >= K && ldx % 8 == 0 && ldw % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0,
                "lav_gemm_skinny_bf16: operands need 16-byte aligned rows (ldx=%ld ldw=%ld)", ldx, ldw);
    LAV_REQUIRE(epi >= LAV_SKINNY_BF16 && epi <= LAV_SKINNY_F32 && ldo >= N, "lav_gemm_skinny_bf16: epi=%d ldo=%ld", epi, ldo);
    LAV_REQUIRE(epi != LAV_SKINNY_RES_F32 || (residual && ldr >= N), "lav_gemm_skinny_bf16: the residual epilogue needs residual rows");
    SkinnyArgs a;
    a.x = (const bf16_t*)x; a.ldx = ldx; a.w = (const bf16_t*)w; a.ldw = ldw; a.M = M; a.N = N; a.K = K; a.bias = bias; a.epi = epi;
    a.res = residual; a.ldr = ldr; a.res_bf16 = residual_bf16; a.out = out; a.ldo = ldo;
    const dim3 grid((N + SK_COLS - 1) / SK_COLS);
    hipStream_t s = (hipStream_t)stream;
    const int mt = (M + 15) / 16;
    if (mt == 1) hipLaunchKernelGGL(skinny_gemm_kernel<1>, grid, dim3(SK_THREADS), 0, s, a);
    else if (mt == 2) hipLaunchKernelGGL(skinny_gemm_kernel<2>, grid, dim3(SK_THREADS), 0, s, a);
    else if (mt == 3) hipLaunchKernelGGL(skinny_gemm_kernel<3>, grid, dim3(SK_THREADS), 0, s, a);
    else hipLaunchKernelGGL(skinny_gemm_kernel<4>, grid, dim3(SK_THREADS), 0, s, a);
    return lav_check_launch("lav_gemm_skinny_bf16");
}

// ---- decode attention --------------------------------------------------------------------------------------------------
#define AD_THREADS 256
#define AD_MAXQ 8
#define AD_HD 64

// key kk of row group b, head h: [0, Lv) video rows of the prefix qkv (those of clip b / beams: the beams of a clip share them in place);
// [Lv, Lv + n_cached) text cache; then the q_len new rows
__device__ __forceinline__ const bf16_t* ad_key(const lav_attn_decode_desc& d, int beams, int b, int h, int kk, int which /* 1 k, 2 v */) {
    const int H = d.heads * AD_HD;
    if (kk < d.Lv) return (const bf16_t*)d.prefix_qkv + ((long)(b / beams) * d.Lv + kk) * d.ld_prefix + which * H + h * AD_HD;
    kk -= d.Lv;
    if (kk < d.n_cached)
        return (const bf16_t*)(which == 1 ? d.cache_k : d.cache_v) + (((long)b * d.heads + h) * d.max_len + kk) * AD_HD;
    kk -= d.n_cached;
    return (const bf16_t*)d.qkv_new + ((long)b * d.q_len + kk) * d.ld_new + which * H + h * AD_HD;
}

__global__ __launch_bounds__(AD_THREADS) void attn_decode_kernel(lav_attn_decode_desc d, int chunk, int beams) {
    extern __shared__ float sh[];
    float* q = sh;                                   // [AD_MAXQ][64] (scaled)
    float* s = q + AD_MAXQ * AD_HD;                  // [q_len][chunk] scores, then probabilities
    float* o4 = s + d.q_len * chunk;                 // [4][q_len][64]
    __shared__ float stat[AD_MAXQ][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bh = blockIdx.x, b = bh / d.heads, h = bh % d.heads, split = blockIdx.y;
    const int H = d.heads * AD_HD;
    const int Lk = d.Lv + d.n_cached + d.q_len;
    const int k0 = split * chunk, k1 = min(Lk, k0 + chunk);
    for (int i = tid; i < d.q_len * AD_HD; i += AD_THREADS) {
        const int j = i / AD_HD, c = i % AD_HD;
        q[i] = bf2f(((const bf16_t*)d.qkv_new)[((long)b * d.q_len + j) * d.ld_new + h * AD_HD + c]) * d.scale;
    }
    // the cache append (rows 0 .. n_append - 1 of the new ones): other workgroups read only positions < n_cached of the cache
    if (split == 0) {
        for (int i = tid; i < d.n_append * AD_HD; i += AD_THREADS) {
            const int j = i / AD_HD, c = i % AD_HD;
            const long src = ((long)b * d.q_len + j) * d.ld_new + h * AD_HD + c;
            const long dst = (((long)b * d.heads + h) * d.max_len + d.n_cached + j) * AD_HD + c;
            ((bf16_t*)d.cache_k)[dst] = ((const bf16_t*)d.qkv_new)[src + H];
            ((bf16_t*)d.cache_v)[dst] = ((const bf16_t*)d.qkv_new)[src + 2 * H];
        }
    }
    __syncthreads();
    // scores: 8 lanes per key (8 dims each), 32 keys per pass
    const int part = tid & 7;
    for (int base = k0; base < k1; base += AD_THREADS / 8) {
        const int kk = base + (tid >> 3);
        const bool live = kk < k1;
        float kf[8];
        if (live) unpack8(*(const uint4*)(ad_key(d, beams, b, h, kk, 1) + part * 8), kf);
        else for (int e = 0; e < 8; ++e) kf[e] = 0.f;
        bool vis_video = true;
        if (live && kk < d.Lv && d.key_mask) vis_video = d.key_mask[(long)(b / beams) * d.Lv + kk] != 0;
        for (int j = 0; j < d.q_len; ++j) {
            float p = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) p = fmaf(q[j * AD_HD + part * 8 + e], kf[e], p);
            p += __shfl_xor(p, 1, 64);
            p += __shfl_xor(p, 2, 64);
            p += __shfl_xor(p, 4, 64);
            const int jn = kk - d.Lv - d.n_cached;          // >= 0: the key of new row jn (causal: visible to rows j >= jn)
            const bool vis = vis_video && (jn < 0 || jn <= j);
            if (live && part == 0) s[j * chunk + (kk - k0)] = vis ? p : -INFINITY;
        }
    }
    __syncthreads();
    const int nk = k1 - k0;
    for (int j = wave; j < d.q_len; j += 4) {
        float m = -INFINITY;
        for (int k = lane; k < nk; k += 64) m = fmaxf(m, s[j * chunk + k]);
        m = wave_max(m);
        float l = 0.f;
        for (int k = lane; k < nk; k += 64) {
            const float v = s[j * chunk + k];
            const float p = v == -INFINITY ? 0.f : __expf(v - m);
            s[j * chunk + k] = p;
            l += p;
        }
        l = wave_sum(l);
        if (lane == 0) { stat[j][0] = m; stat[j][1] = l; }
    }
    __syncthreads();
    // P.V: thread (dim lane, key group wave)
    float acc[AD_MAXQ];
#pragma unroll
    for (int j = 0; j < AD_MAXQ; ++j) acc[j] = 0.f;
    for (int k = wave; k < nk; k += 4) {
        const float v = bf2f(ad_key(d, beams, b, h, k0 + k, 2)[lane]);
#pragma unroll
        for (int j = 0; j < AD_MAXQ; ++j)
            if (j < d.q_len) acc[j] = fmaf(s[j * chunk + k], v, acc[j]);
    }
    for (int j = 0; j < d.q_len; ++j) o4[(wave * d.q_len + j) * AD_HD + lane] = acc[j];
    __syncthreads();
    for (int i = tid; i < d.q_len * AD_HD; i += AD_THREADS) {
        const int j = i / AD_HD, c = i % AD_HD;
        const float o = ((o4[(0 * d.q_len + j) * AD_HD + c] + o4[(1 * d.q_len + j) * AD_HD + c]) + o4[(2 * d.q_len + j) * AD_HD + c]) +
                        o4[(3 * d.q_len + j) * AD_HD + c];
        if (gridDim.y == 1) {
            const float l = stat[j][1];
            ((bf16_t*)d.out)[((long)b * d.q_len + j) * d.ldo + h * AD_HD + c] = f2bf(l > 0.f ? o / l : 0.f);
        } else {
            float* pp = d.partials + (((long)bh * gridDim.y + split) * d.q_len + j) * (AD_HD + 2);
            pp[c] = o;
            if (c == 0) { pp[AD_HD] = stat[j][0]; pp[AD_HD + 1] = stat[j][1]; }
        }
    }
}

__global__ __launch_bounds__(AD_THREADS) void attn_decode_combine_kernel(lav_attn_decode_desc d, int splits) {
    const int bh = blockIdx.x, b = bh / d.heads, h = bh % d.heads;
    for (int i = threadIdx.x; i < d.q_len * AD_HD; i += AD_THREADS) {
        const int j = i / AD_HD, c = i % AD_HD;
        const float* pp = d.partials + ((long)bh * splits * d.q_len + j) * (AD_HD + 2);
        const long st = (long)d.q_len * (AD_HD + 2);
        float m = -INFINITY;
        for (int sp = 0; sp < splits; ++sp) m = fmaxf(m, pp[sp * st + AD_HD]);
        float l = 0.f, o = 0.f;
        for (int sp = 0; sp < splits; ++sp) {
            const float ms = pp[sp * st + AD_HD];
            if (ms == -INFINITY) continue;
            const float f = __expf(ms - m);
            l = fmaf(pp[sp * st + AD_HD + 1], f, l);
            o = fmaf(pp[sp * st + c], f, o);
        }
        ((bf16_t*)d.out)[((long)b * d.q_len + j) * d.ldo + h * AD_HD + c] = f2bf(l > 0.f ? o / l : 0.f);
    }
}

// keys per split: enough workgroups to cover the CUs, at least 16 keys each, at most 1024 (LDS).  The count is a non-decreasing function of the
// key count (Lk = Lv + n_cached + q_len), so a partials workspace sized for the last step of a generation covers every earlier step; the keys are
// cut into `splits` chunks of ceil(Lk / splits), and a trailing chunk may be empty (its partial has max -inf and sum 0: the combine skips it).
static int ad_splits(const lav_attn_decode_desc* d, int* chunk) {
    const int Lk = d->Lv + d->n_cached + d->q_len;
    const int bh = d->B * d->heads;
    int splits = (256 + bh - 1) / bh;
    splits = min(splits, (Lk + 15) / 16);
    splits = max(splits, (Lk + 1023) / 1024);
    splits = max(splits, 1);
    *chunk = (Lk + splits - 1) / splits;
    return splits;
}

extern "C" int lav_attention_decode_splits(const lav_attn_decode_desc* d) {
    if (!d) return 0;
    int chunk;
    return ad_splits(d, &chunk);
}

static int attention_decode(void* stream, const lav_attn_decode_desc* d, int beams) {
    LAV_REQUIRE(d, "lav_attention_decode: null descriptor");
    LAV_REQUIRE(d->head_dim == AD_HD && d->B > 0 && d->heads > 0 && d->q_len >= 1 && d->q_len <= AD_MAXQ && d->Lv >= 0 && d->n_cached >= 0 &&
                d->n_append >= 0 && d->n_append <= d->q_len && d->n_cached + d->n_append <= d->max_len,
                "lav_attention_decode: head_dim=%d (64) B=%d heads=%d q_len=%d (1..8) Lv=%d n_cached=%d n_append=%d max_len=%d", d->head_dim, d->B,
                d->heads, d->q_len, d->Lv, d->n_cached, d->n_append, d->max_len);
    LAV_REQUIRE(d->qkv_new && d->out && (d->Lv == 0 || d->prefix_qkv) && ((d->n_cached + d->n_append) == 0 || (d->cache_k && d->cache_v)),
                "lav_attention_decode: null pointer");
    LAV_REQUIRE(d->ld_new % 8 == 0 && d->ld_prefix % 8 == 0, "lav_attention_decode: row strides must keep 16-byte alignment");
    int chunk;
    const int splits = ad_splits(d, &chunk);
    const long need = (long)d->B * d->heads * splits * d->q_len * (AD_HD + 2);
    if (splits > 1 && (!d->partials || d->partials_capacity < need)) {
        lav_set_error("lav_attention_decode: %d key splits need a partials workspace of %ld floats, %ld given (lav_attention_decode_splits)", splits,
                      need, d->partials ? d->partials_capacity : 0L);
        return LAV_E_WORKSPACE;
    }
    const size_t lds = (size_t)(AD_MAXQ * AD_HD + d->q_len * chunk + 4 * d->q_len * AD_HD) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_decode_kernel, dim3(d->B * d->heads, splits), dim3(AD_THREADS), lds, s, *d, chunk, beams);
    if (int rc = lav_check_launch("lav_attention_decode")) return rc;
    if (splits > 1) {
        hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(d->B * d->heads), dim3(AD_THREADS), 0, s, *d, splits);
        return lav_check_launch("lav_attention_decode (combine)");
    }
    return LAV_OK;
}

extern "C" int lav_attention_decode(void* stream, const lav_attn_decode_desc* d) { return attention_decode(stream, d, 1); }

extern "C" int lav_attention_decode_beam(void* stream, const lav_attn_decode_desc* d, int beams) {
    LAV_REQUIRE(d && beams >= 1 && beams <= LAV_BEAM_MAX && d->B % beams == 0, "lav_attention_decode_beam: beams=%d (1..%d) must divide B=%d", beams,
                LAV_BEAM_MAX, d ? d->B : 0);
    return attention_decode(stream, d, beams);
}

// ---- embeddings of single rows --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_rows_kernel(int n, int Hd, const int64_t* ids, const int32_t* pos_ids, const float* word,
                                                         const float* pos, const float* type0, const float* gamma, const float* beta,
                                                         float eps, bf16_t* out) {
    __shared__ float red[2][4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const long id = ids[r], p = pos_ids[r];
    float v[4];
    float sum = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = it * 256 + tid;
        v[it] = c < Hd ? word[id * Hd + c] + pos[p * Hd + c] + type0[c] : 0.f;
        sum += v[it];
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red[0][tid >> 6] = sum;
    __syncthreads();
    const float mean = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / Hd;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = it * 256 + tid;
        if (c < Hd) { const float dd = v[it] - mean; q += dd * dd; }
    }
    q = wave_sum(q);
    if ((tid & 63) == 0) red[1][tid >> 6] = q;
    __syncthreads();
    const float rstd = rsqrtf((red[1][0] + red[1][1] + red[1][2] + red[1][3]) / Hd + eps);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = it * 256 + tid;
        if (c < Hd) out[(long)r * Hd + c] = f2bf((v[it] - mean) * rstd * gamma[c] + beta[c]);
    }
}

extern "C" int lav_text_embed_rows_fwd(void* stream, int n, int Hd, const int64_t* ids, const int32_t* pos_ids, const float* word,
                                       const float* pos, const float* type0, const float* gamma, const float* beta, float eps, void* out) {
    LAV_REQUIRE(n > 0 && Hd > 0 && Hd <= 1024, "lav_text_embed_rows_fwd: n=%d Hd=%d (<= 1024)", n, Hd);
    LAV_REQUIRE(ids && pos_ids && word && pos && type0 && gamma && beta && out, "lav_text_embed_rows_fwd: null pointer");
    hipLaunchKernelGGL(embed_rows_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, n, Hd, ids, pos_ids, word, pos, type0, gamma, beta, eps,
                       (bf16_t*)out);
    return lav_check_launch("lav_text_embed_rows_fwd");
}

// ---- greedy step ---------------------------------------------------------------------------------------------------------------
#define GS_THREADS 256

__global__ __launch_bounds__(GS_THREADS) void greedy_step_kernel(int V, float* logits, long ld, int64_t* ids, long ld_ids, int cur,
                                                                 float penalty, int32_t* unfinished, float* score_sum, float* count,
                                                                 int64_t pad_id, int64_t eos_id, int64_t* next_ids, long ld_next) {
    __shared__ float sm[GS_THREADS / 64];
    __shared__ int si[GS_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* x = logits + (long)b * ld;
    const int64_t* prev = ids + (long)b * ld_ids;
    if (penalty != 1.f && tid == 0) {
        // every DISTINCT previous id once (model_for_captioning.py:436-447): negative logits are multiplied, the others divided
        for (int c = 0; c < cur; ++c) {
            const int64_t id = prev[c];
            bool seen = false;
            for (int c2 = 0; c2 < c; ++c2) seen |= prev[c2] == id;
            if (seen || id < 0 || id >= V) continue;
            const float v = x[id];
            x[id] = v < 0.f ? v * penalty : v / penalty;
        }
        __threadfence();
    }
    __syncthreads();
    float m = -INFINITY;
    int mi = 0x7fffffff;
    for (int i = tid; i < V; i += GS_THREADS) {
        const float v = x[i];
        if (v > m) { m = v; mi = i; }                      // strided ascending scan: the first maximum of this thread
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64);
        const int i2 = __shfl_xor(mi, o, 64);
        if (m2 > m || (m2 == m && i2 < mi)) { m = m2; mi = i2; }
    }
    if (lane == 0) { sm[wave] = m; si[wave] = mi; }
    __syncthreads();
    m = sm[0]; mi = si[0];
    for (int w = 1; w < GS_THREADS / 64; ++w)
        if (sm[w] > m || (sm[w] == m && si[w] < mi)) { m = sm[w]; mi = si[w]; }
    __syncthreads();
    float l = 0.f;
    for (int i = tid; i < V; i += GS_THREADS) l += __expf(x[i] - m);
    l = wave_sum(l);
    if (lane == 0) sm[wave] = l;
    __syncthreads();
    if (tid == 0) {
        l = (sm[0] + sm[1]) + (sm[2] + sm[3]);
        if (mi >= V) mi = 0;                               // every logit NaN / -inf: nothing to pick; keep the index in range
        const float score = x[mi] - m - logf(l);
        const int u = unfinished[b];
        const int64_t tok = u ? (int64_t)mi : pad_id;
        ids[(long)b * ld_ids + cur] = tok;
        if (next_ids) next_ids[(long)b * ld_next] = tok;
        score_sum[b] += u ? score : 0.f;
        count[b] += u ? 1.f : 0.f;
        unfinished[b] = (u && tok != eos_id) ? 1 : 0;
    }
}

extern "C" int lav_greedy_step(void* stream, int B, int V, float* logits, long ld, int64_t* ids, long ld_ids, int cur, float penalty,
                               int32_t* unfinished, float* score_sum, float* count, int64_t pad_id, int64_t eos_id, int64_t* next_ids, long ld_next) {
    LAV_REQUIRE(B > 0 && V > 0 && ld >= V && cur >= 1 && cur < ld_ids, "lav_greedy_step: B=%d V=%d ld=%ld cur=%d ld_ids=%ld", B, V, ld, cur, ld_ids);
    LAV_REQUIRE(logits && ids && unfinished && score_sum && count, "lav_greedy_step: null pointer");
    LAV_REQUIRE(penalty > 0.f, "lav_greedy_step: penalty must be positive");
    hipLaunchKernelGGL(greedy_step_kernel, dim3(B), dim3(GS_THREADS), 0, (hipStream_t)stream, V, logits, ld, ids, ld_ids, cur, penalty,
                       unfinished, score_sum, count, pad_id, eos_id, next_ids, ld_next);
    return lav_check_launch("lav_greedy_step");
}

// ---- beam search ---------------------------------------------------------------------------------------------------------------
// The beam search of Oscar / SwinBERT's _generate_beam_search + BeamHypotheses (HF 2.x) on the device: no host synchronisation per step.
#define BS_THREADS 256
#define BS_TOP (2 * LAV_BEAM_MAX)           // the running top list of each thread: 2 * beams candidates per row at most

// candidate order: value descending, index ascending on a tie
__device__ __forceinline__ bool bs_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// (m, s) = running max and sum of exp(x - m); merge of two such pairs
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) return;
    s = (m == -INFINITY ? 0.f : s * __expf(m - M)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - M));
    m = M;
}

__global__ __launch_bounds__(BS_THREADS) void beam_step_kernel(int V, float* logits, long ld, const int64_t* ids, long ld_ids, int cur,
                                                               float penalty, const float* beam_scores, int k, float* cand_score,
                                                               int32_t* cand_word) {
    __shared__ float sv[BS_THREADS / 64], sm[BS_THREADS / 64], ss[BS_THREADS / 64];
    __shared__ int si[BS_THREADS / 64];
    __shared__ float top_v[BS_TOP];
    __shared__ int top_i[BS_TOP];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* x = logits + (long)r * ld;
    const int64_t* prev = ids + (long)r * ld_ids;
    if (penalty != 1.f && tid == 0) {
        // this beam's DISTINCT previous ids once, in place (the rule of lav_greedy_step)
        for (int c = 0; c < cur; ++c) {
            const int64_t id = prev[c];
            bool seen = false;
            for (int c2 = 0; c2 < c; ++c2) seen |= prev[c2] == id;
            if (seen || id < 0 || id >= V) continue;
            const float v = x[id];
            x[id] = v < 0.f ? v * penalty : v / penalty;
        }
        __threadfence();
    }
    __syncthreads();
    // one pass: online max / sum-exp and this thread's top BS_TOP (its indices ascend, so a kept entry never ties a later one from below)
    float tv[BS_TOP];
    int ti[BS_TOP];
#pragma unroll
    for (int j = 0; j < BS_TOP; ++j) { tv[j] = -INFINITY; ti[j] = 0x7fffffff; }
    float m = -INFINITY, s = 0.f;
    for (int i = tid; i < V; i += BS_THREADS) {
        const float v = x[i];
        if (v > m) { s = s * __expf(m - v) + 1.f; m = v; }
        else if (v > -INFINITY) s += __expf(v - m);
        if (bs_better(v, i, tv[BS_TOP - 1], ti[BS_TOP - 1])) {
#pragma unroll
            for (int j = BS_TOP - 1; j > 0; --j) {
                if (bs_better(v, i, tv[j - 1], ti[j - 1])) { tv[j] = tv[j - 1]; ti[j] = ti[j - 1]; }
                else if (bs_better(v, i, tv[j], ti[j])) { tv[j] = v; ti[j] = i; }
            }
            if (bs_better(v, i, tv[0], ti[0])) { tv[0] = v; ti[0] = i; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    if (lane == 0) { sm[wave] = m; ss[wave] = s; }
    // k rounds: the best head of all threads' lists is the next candidate; its owner pops it
    for (int j = 0; j < k; ++j) {
        float bv = tv[0];
        int bi = ti[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(bv, o, 64);
            const int i2 = __shfl_xor(bi, o, 64);
            if (bs_better(v2, i2, bv, bi)) { bv = v2; bi = i2; }
        }
        if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
        __syncthreads();
        bv = sv[0]; bi = si[0];
        for (int w = 1; w < BS_THREADS / 64; ++w)
            if (bs_better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
        if (ti[0] == bi) {
#pragma unroll
            for (int q = 0; q < BS_TOP - 1; ++q) { tv[q] = tv[q + 1]; ti[q] = ti[q + 1]; }
            tv[BS_TOP - 1] = -INFINITY; ti[BS_TOP - 1] = 0x7fffffff;
        }
        if (tid == 0) { top_v[j] = bv; top_i[j] = bi; }
        __syncthreads();
    }
    if (tid < k) {
        float M = sm[0], S = ss[0];
        for (int w = 1; w < BS_THREADS / 64; ++w) lse_merge(M, S, sm[w], ss[w]);
        const int w = min(top_i[tid], V - 1);                   // V >= k: never clamped for finite rows
        cand_score[(long)r * k + tid] = (top_v[tid] - M) - logf(S) + beam_scores[r];
        cand_word[(long)r * k + tid] = w;
    }
}

extern "C" int lav_beam_step(void* stream, int rows, int beams, int V, float* logits, long ld, const int64_t* ids, long ld_ids, int cur,
                             float penalty, const float* beam_scores, float* cand_score, int32_t* cand_word) {
    LAV_REQUIRE(rows > 0 && beams >= 1 && beams <= LAV_BEAM_MAX && V >= 2 * beams && ld >= V && cur >= 1 && cur <= ld_ids,
                "lav_beam_step: rows=%d beams=%d (1..%d) V=%d ld=%ld cur=%d ld_ids=%ld", rows, beams, LAV_BEAM_MAX, V, ld, cur, ld_ids);
    LAV_REQUIRE(logits && ids && beam_scores && cand_score && cand_word, "lav_beam_step: null pointer");
    LAV_REQUIRE(penalty > 0.f, "lav_beam_step: penalty must be positive");
    hipLaunchKernelGGL(beam_step_kernel, dim3(rows), dim3(BS_THREADS), 0, (hipStream_t)stream, V, logits, ld, ids, ld_ids, cur, penalty,
                       beam_scores, 2 * beams, cand_score, cand_word);
    return lav_check_launch("lav_beam_step");
}

#define SEL_THREADS 128                     // >= LAV_BEAM_MAX * 2 * LAV_BEAM_MAX candidates of a clip

__global__ __launch_bounds__(SEL_THREADS) void beam_select_kernel(lav_beam_select_desc d) {
    extern __shared__ int64_t par_ids[];                     // [beams][cur]: the next beams' parent ids
    __shared__ float c_s[2 * LAV_BEAM_MAX];
    __shared__ int c_beam[2 * LAV_BEAM_MAX];
    __shared__ int64_t c_word[2 * LAV_BEAM_MAX];
    __shared__ int n_par[LAV_BEAM_MAX];
    __shared__ int64_t n_word[LAV_BEAM_MAX];
    __shared__ float n_score[LAV_BEAM_MAX];
    __shared__ int slot_src[LAV_BEAM_MAX];
    const int c = blockIdx.x, tid = threadIdx.x, nb = d.beams, k2 = 2 * nb, n = nb * k2, cur = d.cur, L = d.max_len;
    const long row0 = (long)c * nb;
    if (tid < k2) { c_s[tid] = -INFINITY; c_beam[tid] = 0; c_word[tid] = d.pad_id; }
    __syncthreads();
    // merge: every candidate's rank in the clip (score descending, flat index beam * V + word ascending)
    if (tid < n) {
        const float v = d.cand_score[(row0 + tid / k2) * k2 + tid % k2];
        const long f = (long)(tid / k2) * d.V + d.cand_word[(row0 + tid / k2) * k2 + tid % k2];
        int rank = 0;
        for (int o = 0; o < n; ++o) {
            const float v2 = d.cand_score[(row0 + o / k2) * k2 + o % k2];
            const long f2 = (long)(o / k2) * d.V + d.cand_word[(row0 + o / k2) * k2 + o % k2];
            rank += (v2 > v || (v2 == v && f2 < f)) ? 1 : 0;
        }
        if (rank < k2) { c_s[rank] = v; c_beam[rank] = tid / k2; c_word[rank] = f - (long)(tid / k2) * d.V; }
    }
    __syncthreads();
    if (tid == 0) {
        int* st = d.state + 3 * c;                           // held, done, insertions so far
        int held = st[0], done = st[1], seq = st[2];
        float worst = d.worst[c];
        float* hs = d.hyp_score + (long)c * d.keep;
        int* hq = d.hyp_seq + (long)c * d.keep;
        for (int j = 0; j < d.keep; ++j) slot_src[j] = -1;
        for (int b = 0; b < nb; ++b) { n_par[b] = b; n_word[b] = d.pad_id; n_score[b] = d.beam_scores[row0 + b]; }
        if (!done && held == d.keep && (d.early_stopping || worst >= c_s[0] / d.max_norm)) done = 1;
        if (!done) {
            const bool last = cur + 1 == L;
            int nn = 0;
            for (int j = 0; j < k2 && nn < nb; ++j) {
                if (c_word[j] == d.eos_id || last) {
                    const float sc = c_s[j] / d.cur_norm;
                    if (held < d.keep) {                             // a plain add
                        hs[held] = sc; hq[held] = seq++; slot_src[held] = c_beam[j];
                        ++held;
                        worst = fminf(worst, sc);
                    } else if (sc > worst) {                         // overflow: the lowest score goes, the earliest insertion among equals
                        int slot = 0;
                        for (int q = 1; q < d.keep; ++q)
                            if (hs[q] < hs[slot] || (hs[q] == hs[slot] && hq[q] < hq[slot])) slot = q;
                        hs[slot] = sc; hq[slot] = seq++; slot_src[slot] = c_beam[j];
                        worst = hs[0];
                        for (int q = 1; q < d.keep; ++q) worst = fminf(worst, hs[q]);
                    }
                } else {
                    n_par[nn] = c_beam[j]; n_word[nn] = c_word[j]; n_score[nn] = c_s[j];
                    ++nn;
                }
            }
        }
        st[0] = held; st[1] = done; st[2] = seq;
        d.worst[c] = worst;
    }
    __syncthreads();
    // hypothesis rows written this step: the parent's ids [0, cur), [SEP], then [PAD]
    for (int j = 0; j < d.keep; ++j) {
        const int src = slot_src[j];
        if (src < 0) continue;
        const int64_t* p = d.ids + (row0 + src) * d.ld_ids;
        int64_t* h = d.hyp_ids + ((long)c * d.keep + j) * L;
        for (int q = tid; q < L; q += SEL_THREADS) h[q] = q < cur ? p[q] : (q == cur ? d.eos_id : d.pad_id);
    }
    for (int i = tid; i < nb * cur; i += SEL_THREADS) par_ids[i] = d.ids[(row0 + n_par[i / cur]) * d.ld_ids + i % cur];
    __syncthreads();
    for (int i = tid; i < nb * cur; i += SEL_THREADS) d.ids[(row0 + i / cur) * d.ld_ids + i % cur] = par_ids[i];
    if (tid < nb) {
        const long r = row0 + tid;
        d.ids[r * d.ld_ids + cur] = n_word[tid];
        if (d.next_ids) d.next_ids[r * d.ld_next] = n_word[tid];
        d.parent[r] = (int32_t)(row0 + n_par[tid]);
        d.beam_scores[r] = n_score[tid];
    }
}

extern "C" int lav_beam_select(void* stream, const lav_beam_select_desc* d) {
    LAV_REQUIRE(d, "lav_beam_select: null descriptor");
    LAV_REQUIRE(d->clips > 0 && d->beams >= 1 && d->beams <= LAV_BEAM_MAX && d->keep >= 1 && d->keep <= d->beams && d->V >= 2 * d->beams &&
                d->max_len >= 2 && d->max_len <= 512 && d->cur >= 1 && d->cur < d->max_len && d->ld_ids >= d->max_len,
                "lav_beam_select: clips=%d beams=%d (1..%d) keep=%d (1..beams) V=%d max_len=%d (2..512) cur=%d ld_ids=%ld", d->clips, d->beams,
                LAV_BEAM_MAX, d->keep, d->V, d->max_len, d->cur, d->ld_ids);
    LAV_REQUIRE(d->cur_norm > 0.f && d->max_norm > 0.f, "lav_beam_select: the length normalisers must be positive");
    LAV_REQUIRE(d->cand_score && d->cand_word && d->beam_scores && d->ids && d->parent && d->hyp_ids && d->hyp_score && d->hyp_seq && d->state &&
                d->worst, "lav_beam_select: null pointer");
    const size_t lds = (size_t)d->beams * d->cur * sizeof(int64_t);
    hipLaunchKernelGGL(beam_select_kernel, dim3(d->clips), dim3(SEL_THREADS), lds, (hipStream_t)stream, *d);
    return lav_check_launch("lav_beam_select");
}

// one workgroup per (row, head) of one layer's k or v: positions [0, n_pos) of row parent[row] of the source cache
__global__ __launch_bounds__(128) void beam_reparent_kernel(lav_beam_reparent_desc d) {
    const int rh = blockIdx.x, r = rh / d.heads, h = rh % d.heads, layer = blockIdx.y, which = blockIdx.z;
    int p = d.parent[r];
    if (p < 0 || p >= d.rows) p = r;
    const uint4* src = (const uint4*)(which ? d.src_v[layer] : d.src_k[layer]) + ((long)p * d.heads + h) * d.max_len * (AD_HD / 8);
    uint4* dst = (uint4*)(which ? d.dst_v[layer] : d.dst_k[layer]) + ((long)r * d.heads + h) * d.max_len * (AD_HD / 8);
    for (int i = threadIdx.x; i < d.n_pos * (AD_HD / 8); i += 128) dst[i] = src[i];
}

extern "C" int lav_beam_reparent(void* stream, const lav_beam_reparent_desc* d) {
    LAV_REQUIRE(d, "lav_beam_reparent: null descriptor");
    LAV_REQUIRE(d->layers >= 1 && d->layers <= LAV_REPARENT_MAX_LAYERS && d->rows > 0 && d->heads > 0 && d->n_pos >= 0 && d->n_pos <= d->max_len,
                "lav_beam_reparent: layers=%d (1..%d) rows=%d heads=%d n_pos=%d max_len=%d", d->layers, LAV_REPARENT_MAX_LAYERS, d->rows, d->heads,
                d->n_pos, d->max_len);
    LAV_REQUIRE(d->parent, "lav_beam_reparent: null parent");
    for (int l = 0; l < d->layers; ++l) {
        LAV_REQUIRE(d->src_k[l] && d->src_v[l] && d->dst_k[l] && d->dst_v[l], "lav_beam_reparent: null cache of layer %d", l);
        LAV_REQUIRE(((uintptr_t)d->src_k[l] | (uintptr_t)d->src_v[l] | (uintptr_t)d->dst_k[l] | (uintptr_t)d->dst_v[l]) % 16 == 0,
                    "lav_beam_reparent: caches must be 16-byte aligned");
    }
    if (d->n_pos == 0) return LAV_OK;
    hipLaunchKernelGGL(beam_reparent_kernel, dim3(d->rows * d->heads, d->layers, 2), dim3(128), 0, (hipStream_t)stream, *d);
    return lav_check_launch("lav_beam_reparent");
}
