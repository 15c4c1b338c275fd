// Memory-bound edge kernels of the LAVENDER path: patch im2col, video-token assembly (+LN), text embedding
// (+LN +dropout), and the row gathers that build / un-build the fusion-encoder input.  One wave per row,
// 16-byte accesses.
#include "common.h"
#include "../../include/lavender_hip.h"

// ---- PatchEmbed3D im2col (video_swin.py:388-405) -----------------------------------------------------
__global__ __launch_bounds__(256) void im2col_kernel(const float* __restrict__ img, int B, int T, int H, int W, int frame_major,
                                                    bf16_t* __restrict__ out) {
    const int Hp = H >> 2, Wp = W >> 2;
    const long total = (long)B * T * Hp * 12 * Wp;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        int pw = idx % Wp; long t1 = idx / Wp;
        int chunk = t1 % 12; t1 /= 12;
        int ph = t1 % Hp; t1 /= Hp;
        int t = t1 % T, b = t1 / T;
        int c = chunk >> 2, kt = (chunk >> 1) & 1, khp = chunk & 1;
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int ts = t + kt;
        if (ts < T) {                                    // zero frame appended at the END of T (:396)
            const long plane = frame_major ? (((long)b * T + ts) * 3 + c) : (((long)b * 3 + c) * T + ts);
            const float* p = img + plane * H * W + (long)(4 * ph + 2 * khp) * W + 4 * pw;
            float4 r0 = *(const float4*)p, r1 = *(const float4*)(p + W);
            v[0] = r0.x; v[1] = r0.y; v[2] = r0.z; v[3] = r0.w; v[4] = r1.x; v[5] = r1.y; v[6] = r1.z; v[7] = r1.w;
        }
        const long row = (((long)b * T + t) * Hp + ph) * Wp + pw;
        *(uint4*)(out + row * 96 + c * 32 + kt * 16 + khp * 8) = pack8(v);
    }
}

extern "C" int lav_patch_im2col(void* stream, const float* img, int B, int T, int H, int W, int frame_major, void* out) {
    LAV_REQUIRE(img && out && B > 0 && T > 0, "lav_patch_im2col: bad arguments");
    LAV_REQUIRE(H % 4 == 0 && W % 4 == 0, "lav_patch_im2col: H,W must be multiples of the 4x4 patch (got %d,%d)", H, W);
    long total = (long)B * T * (H / 4) * 12 * (W / 4);
    int grid = (int)((total + 255) / 256 > 65535 ? 65535 : (total + 255) / 256);
    hipLaunchKernelGGL(im2col_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, img, B, T, H, W, frame_major, (bf16_t*)out);
    return lav_check_launch("lav_patch_im2col");
}

// ---- video token assembly + LayerNorm (model.py:69-85) -----------------------------------------------
// MAXC = chunks (of 8) per lane: Hd <= 64*8*MAXC
template <int MAXC>
__global__ __launch_bounds__(256) void video_embed_fwd_kernel(int B, int T, int hw, int Hd, const bf16_t* __restrict__ feat,
                                                             const float* cls, const float* pos, const float* len,
                                                             const float* gamma, const float* beta, float eps,
                                                             bf16_t* __restrict__ out, long seq_rows, float* mean_o, float* rstd_o) {
    const int lane = threadIdx.x & 63;
    const int P = 1 + hw;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long)B * T * P) return;
    const int pp = r % P; const int bt = r / P; const int t = bt % T, b = bt / T;
    float v[MAXC][8];
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
        const int col = (it * 64 + lane) * 8;
        if (col < Hd) {
            float x[8];
            if (pp == 0) { for (int k = 0; k < 8; ++k) x[k] = cls[col + k]; }
            else { uint4 u = *(const uint4*)(feat + ((long)bt * hw + pp - 1) * Hd + col); unpack8(u, x); }
#pragma unroll
            for (int k = 0; k < 8; ++k) { v[it][k] = x[k] + pos[(long)pp * Hd + col + k] + len[(long)t * Hd + col + k]; s += v[it][k]; }
        }
    }
    const float mean = wave_sum(s) / Hd;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
        const int col = (it * 64 + lane) * 8;
        if (col < Hd) {
#pragma unroll
            for (int k = 0; k < 8; ++k) { float d = v[it][k] - mean; q += d * d; }
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / Hd + eps);
    bf16_t* o = out + ((long)b * seq_rows + (long)t * P + pp) * Hd;
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
        const int col = (it * 64 + lane) * 8;
        if (col < Hd) {
            float y[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) y[k] = (v[it][k] - mean) * rstd * gamma[col + k] + beta[col + k];
            *(uint4*)(o + col) = pack8(y);
        }
    }
    if (lane == 0) { mean_o[r] = mean; rstd_o[r] = rstd; }
}

// backward: one block per (token position p' (0 = cls), frame t); its four waves take the B rows that share the position and length
// embeddings round-robin, a row per wave: 16-byte accesses (a lane owns 8-column chunks lane, lane + 64), row statistics by wave
// reductions -- no block barrier in the row loop (round 5: the first form walked the rows one by one with 2-byte loads and two
// __syncthreads per row: 236 us for 37 MB).  d_pos[p'], d_len[t], dgamma and dbeta are register sums per wave, merged through LDS: one atomic
// per element per block.
__global__ __launch_bounds__(256) void video_embed_bwd_kernel(int B, int T, int hw, int Hd, const bf16_t* __restrict__ dout, long seq_rows,
                                                             const bf16_t* __restrict__ feat, const float* cls, const float* pos,
                                                             const float* len, const float* gamma, const float* mean_i,
                                                             const float* rstd_i, bf16_t* __restrict__ dfeat, float* d_cls, float* d_pos,
                                                             float* d_len, float* dgamma, float* dbeta) {
    __shared__ float red[3][3][1024];                        // waves 1..3: (d_pos = d_len sum, dgamma, dbeta) per column
    const int P = 1 + hw, pp = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int MAXC = 2;                                   // 8-column chunks per lane: Hd <= 1024
    float xe[MAXC][8], gam[MAXC][8], a_x[MAXC][8], a_g[MAXC][8], a_b[MAXC][8];
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
        const int col = (it * 64 + lane) * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool ok = col < Hd;
            xe[it][k] = ok ? pos[(long)pp * Hd + col + k] + (pp == 0 ? cls[col + k] : 0.f) + len[(long)t * Hd + col + k] : 0.f;
            gam[it][k] = ok ? gamma[col + k] : 0.f;
            a_x[it][k] = a_g[it][k] = a_b[it][k] = 0.f;
        }
    }
    for (int b = wave; b < B; b += 4) {
        const int bt = b * T + t;
        const long r = (long)bt * P + pp;
        const float mean = mean_i[r], rstd = rstd_i[r];
        const bf16_t* dy = dout + ((long)b * seq_rows + (long)t * P + pp) * Hd;
        const bf16_t* fr = feat + ((long)bt * hw + (pp > 0 ? pp - 1 : 0)) * Hd;
        float xh[MAXC][8], gy[MAXC][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int it = 0; it < MAXC; ++it) {
            const int col = (it * 64 + lane) * 8;
            if (col < Hd) {
                float d[8], f[8];
                unpack8(*(const uint4*)(dy + col), d);
                if (pp > 0) unpack8(*(const uint4*)(fr + col), f);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    xh[it][k] = ((pp > 0 ? f[k] : 0.f) + xe[it][k] - mean) * rstd;
                    gy[it][k] = gam[it][k] * d[k];
                    s1 += gy[it][k]; s2 += gy[it][k] * xh[it][k];
                    a_g[it][k] += d[k] * xh[it][k]; a_b[it][k] += d[k];
                }
            }
        }
        const float m1 = wave_sum(s1) / Hd, m2 = wave_sum(s2) / Hd;
#pragma unroll
        for (int it = 0; it < MAXC; ++it) {
            const int col = (it * 64 + lane) * 8;
            if (col < Hd) {
                float dx[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) { dx[k] = rstd * (gy[it][k] - m1 - xh[it][k] * m2); a_x[it][k] += dx[k]; }
                if (pp > 0) *(uint4*)(dfeat + ((long)bt * hw + pp - 1) * Hd + col) = pack8(dx);
            }
        }
    }
    // merge the four waves' column sums, then one atomic per element per block
    if (wave > 0) {
#pragma unroll
        for (int it = 0; it < MAXC; ++it) {
            const int col = (it * 64 + lane) * 8;
            if (col < Hd)
#pragma unroll
                for (int k = 0; k < 8; ++k) { red[wave - 1][0][col + k] = a_x[it][k]; red[wave - 1][1][col + k] = a_g[it][k]; red[wave - 1][2][col + k] = a_b[it][k]; }
        }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int it = 0; it < MAXC; ++it) {
            const int col = (it * 64 + lane) * 8;
            if (col < Hd)
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int c = col + k;
                    const float sx = a_x[it][k] + red[0][0][c] + red[1][0][c] + red[2][0][c];
                    const float sg = a_g[it][k] + red[0][1][c] + red[1][1][c] + red[2][1][c];
                    const float sb = a_b[it][k] + red[0][2][c] + red[1][2][c] + red[2][2][c];
                    atomicAdd(d_len + (long)t * Hd + c, sx);
                    atomicAdd(d_pos + (long)pp * Hd + c, sx);
                    if (pp == 0) atomicAdd(d_cls + c, sx);
                    atomicAdd(dgamma + c, sg);
                    atomicAdd(dbeta + c, sb);
                }
        }
    }
}

extern "C" int lav_video_embed_fwd(void* stream, int B, int T, int hw, int Hd, const void* feat, const float* emb_cls,
                                   const float* emb_pos, const float* emb_len, const float* gamma, const float* beta,
                                   float eps, void* out, long seq_rows, float* mean, float* rstd) {
    LAV_REQUIRE(B > 0 && T > 0 && hw > 0 && Hd % 8 == 0 && Hd <= 1024, "lav_video_embed_fwd: bad shape (Hd=%d)", Hd);
    LAV_REQUIRE(feat && emb_cls && emb_pos && emb_len && gamma && beta && out && mean && rstd, "lav_video_embed_fwd: null pointer");
    long rows = (long)B * T * (1 + hw);
    hipLaunchKernelGGL(video_embed_fwd_kernel<2>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, B, T, hw, Hd,
                       (const bf16_t*)feat, emb_cls, emb_pos, emb_len, gamma, beta, eps, (bf16_t*)out, seq_rows, mean, rstd);
    return lav_check_launch("lav_video_embed_fwd");
}

extern "C" int lav_video_embed_bwd(void* stream, int B, int T, int hw, int Hd, const void* dout, long seq_rows, const void* feat,
                                   const float* emb_cls, const float* emb_pos, const float* emb_len, const float* gamma,
                                   const float* mean, const float* rstd, void* dfeat, float* d_cls, float* d_pos, float* d_len,
                                   float* dgamma, float* dbeta) {
    LAV_REQUIRE(B > 0 && T > 0 && hw > 0 && Hd % 8 == 0 && Hd <= 1024, "lav_video_embed_bwd: bad shape (Hd=%d)", Hd);
    LAV_REQUIRE(dout && feat && dfeat && d_cls && d_pos && d_len && dgamma && dbeta, "lav_video_embed_bwd: null pointer");
    hipLaunchKernelGGL(video_embed_bwd_kernel, dim3(1 + hw, T), dim3(256), 0, (hipStream_t)stream, B, T, hw, Hd,
                       (const bf16_t*)dout, seq_rows, (const bf16_t*)feat, emb_cls, emb_pos, emb_len, gamma, mean, rstd,
                       (bf16_t*)dfeat, d_cls, d_pos, d_len, dgamma, dbeta);
    return lav_check_launch("lav_video_embed_bwd");
}

// ---- BERT text embedding (+LN eps, +dropout) ---------------------------------------------------------
// Lp > 0 (lav_text_embed_pre_fwd): text j's block of `out` is Lp + X rows [pre-text ; text]; text row r = j * X + x lands at row
// r + (j + 1) * Lp, its dropout key and mean / rstd index stay r (the bits of lav_text_embed_fwd).  The waves past the n * X text rows copy
// the n * Lp pre-text rows from pre + j * pre_stride.
template <int MAXC>
__global__ __launch_bounds__(256) void text_embed_fwd_kernel(int n, int X, int Hd, const int64_t* ids, const float* word, const float* pos,
                                                            const float* type0, const float* gamma, const float* beta, float eps,
                                                            float p, uint32_t seed, uint32_t thresh, bf16_t* out, float* mean_o,
                                                            float* rstd_o, int Lp, const bf16_t* pre, long pre_stride) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long)n * X) {
        const long q = r - (long)n * X;
        if (q >= (long)n * Lp) return;
        const long j = q / Lp, pp = q - j * Lp;
        const bf16_t* src = pre + j * pre_stride + pp * Hd;
        bf16_t* dst = out + (j * (Lp + X) + pp) * Hd;
#pragma unroll
        for (int it = 0; it < MAXC; ++it) {
            const int col = (it * 64 + lane) * 8;
            if (col < Hd) *(uint4*)(dst + col) = *(const uint4*)(src + col);
        }
        return;
    }
    const int xp = r % X;
    const long ro = r + (r / X + 1) * Lp;               // output row j * (Lp + X) + Lp + x (r when Lp = 0)
    const long id = ids[r];
    float v[MAXC][8];
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
        const int col = (it * 64 + lane) * 8;
        if (col < Hd) {
#pragma unroll
            for (int k = 0; k < 8; ++k) { v[it][k] = word[id * Hd + col + k] + pos[(long)xp * Hd + col + k] + type0[col + k]; s += v[it][k]; }
        }
    }
    const float mean = wave_sum(s) / Hd;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
        const int col = (it * 64 + lane) * 8;
        if (col < Hd) {
#pragma unroll
            for (int k = 0; k < 8; ++k) { float d = v[it][k] - mean; q += d * d; }
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / Hd + eps);
    const float inv = p > 0.f ? 1.f / (1.f - p) : 1.f;
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
        const int col = (it * 64 + lane) * 8;
        if (col < Hd) {
            float y[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                y[k] = (v[it][k] - mean) * rstd * gamma[col + k] + beta[col + k];
                if (p > 0.f) y[k] = lav_keep(seed, (uint32_t)r * (uint32_t)Hd + (uint32_t)(col + k), thresh) ? y[k] * inv : 0.f;
            }
            *(uint4*)(out + ro * Hd + col) = pack8(y);
        }
    }
    if (lane == 0) { mean_o[r] = mean; rstd_o[r] = rstd; }
}

// Pre-text gradient of one pre-text row p over the texts [s0, s1e) of a block (the blocks past the X text positions of text_embed_bwd_kernel).
//   pre_stride != 0 (a block per text): d_pre is bf16 (n, Lp, Hd) and takes text j's rows as they are.
//   pre_stride == 0 (one broadcast block): sum_j dout[j, p] in fp32, in a FIXED order -- each wave its texts s0 + wave, s0 + wave + 4, ...
//   in turn, then waves 0 + 1 + 2 + 3 -- and no atomics: run to run the same bits.  One group (gridDim.y == 1) finishes here (mode 0: fp32
//   d_pre[p] += sum, mode 1: bf16 d_pre[p] = sum); several groups leave fp32 partials part[group][p] for text_pre_grad_finish_kernel.
__device__ __forceinline__ void text_pre_grad(int n, int X, int Hd, const bf16_t* dout, int Lp, int p, int s0, int s1e, long pre_stride,
                                              void* d_pre, int mode, float* part, float* red) {
    constexpr int MAXC = 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (pre_stride != 0) {
        for (int sq = s0 + wave; sq < s1e; sq += 4) {
            const bf16_t* src = dout + ((long)sq * (Lp + X) + p) * Hd;
            bf16_t* dst = (bf16_t*)d_pre + ((long)sq * Lp + p) * Hd;
#pragma unroll
            for (int it = 0; it < MAXC; ++it) {
                const int col = (it * 64 + lane) * 8;
                if (col < Hd) *(uint4*)(dst + col) = *(const uint4*)(src + col);
            }
        }
        return;
    }
    float a[MAXC][8];
#pragma unroll
    for (int it = 0; it < MAXC; ++it)
#pragma unroll
        for (int k = 0; k < 8; ++k) a[it][k] = 0.f;
    for (int sq = s0 + wave; sq < s1e; sq += 4) {
        const bf16_t* src = dout + ((long)sq * (Lp + X) + p) * Hd;
#pragma unroll
        for (int it = 0; it < MAXC; ++it) {
            const int col = (it * 64 + lane) * 8;
            if (col < Hd) {
                float d[8];
                unpack8(*(const uint4*)(src + col), d);
#pragma unroll
                for (int k = 0; k < 8; ++k) a[it][k] += d[k];
            }
        }
    }
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
        const int col = (it * 64 + lane) * 8;
        if (col < Hd)
#pragma unroll
            for (int k = 0; k < 8; ++k) red[wave * Hd + col + k] = a[it][k];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < Hd; c += 256) {
        const float v = ((red[c] + red[Hd + c]) + red[2 * Hd + c]) + red[3 * Hd + c];
        if (gridDim.y > 1) part[((long)blockIdx.y * Lp + p) * Hd + c] = v;
        else if (mode == 0) ((float*)d_pre)[(long)p * Hd + c] += v;
        else ((bf16_t*)d_pre)[(long)p * Hd + c] = f2bf(v);
    }
}

// the groups' partials of the broadcast pre-text gradient, summed in group order: one block per pre-text row
__global__ __launch_bounds__(256) void text_pre_grad_finish_kernel(int groups, int Lp, int Hd, const float* __restrict__ part, void* d_pre,
                                                                  int mode) {
    const int p = blockIdx.x;
    for (int c = threadIdx.x; c < Hd; c += 256) {
        float v = 0.f;
        for (int g = 0; g < groups; ++g) v += part[((long)g * Lp + p) * Hd + c];
        if (mode == 0) ((float*)d_pre)[(long)p * Hd + c] += v;
        else ((bf16_t*)d_pre)[(long)p * Hd + c] = f2bf(v);
    }
}

// backward: one block per (token position, group of sequences): the rows of a block share the position embedding, so
// d_pos[x], d_type0, dgamma and dbeta are accumulated in registers, merged across the four waves through LDS and
// flushed with ONE atomic per column per block (the per-row version issued 5 same-address atomics per element);
// only the word-embedding rows are scattered per row.
template <int MAXC>
__global__ __launch_bounds__(256) void text_embed_bwd_kernel(int n, int X, int Hd, const int64_t* ids, const bf16_t* dout, const float* word,
                                                            const float* pos, const float* type0, const float* gamma,
                                                            const float* mean_i, const float* rstd_i, float p, uint32_t seed,
                                                            uint32_t thresh, float* d_word, float* d_pos, float* d_type0,
                                                            float* dgamma, float* dbeta, int Lp, long pre_stride, void* d_pre,
                                                            int d_pre_mode, float* part) {
    extern __shared__ float red[];                        // [4 waves][3][Hd]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int xp = blockIdx.x;
    const int per = (n + gridDim.y - 1) / gridDim.y;
    const int s0 = blockIdx.y * per, s1e = min(n, s0 + per);
    if (xp >= X) {                                        // pre-text row xp - X (lav_text_embed_pre_bwd)
        text_pre_grad(n, X, Hd, dout, Lp, xp - X, s0, s1e, pre_stride, d_pre, d_pre_mode, part, red);
        return;
    }
    const float inv = p > 0.f ? 1.f / (1.f - p) : 1.f;
    float a_g[MAXC][8], a_b[MAXC][8], a_x[MAXC][8];
#pragma unroll
    for (int it = 0; it < MAXC; ++it)
#pragma unroll
        for (int k = 0; k < 8; ++k) { a_g[it][k] = 0.f; a_b[it][k] = 0.f; a_x[it][k] = 0.f; }
    for (int sq = s0 + wave; sq < s1e; sq += 4) {
        const long r = (long)sq * X + xp;
        const long id = ids[r];
        const float mean = mean_i[r], rstd = rstd_i[r];
        float xh[MAXC][8], gy[MAXC][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int it = 0; it < MAXC; ++it) {
            const int col = (it * 64 + lane) * 8;
            if (col < Hd) {
                float d[8];
                uint4 du = *(const uint4*)(dout + (r + (long)(sq + 1) * Lp) * Hd + col); unpack8(du, d);   // row sq * (Lp + X) + Lp + xp
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (p > 0.f) d[k] = lav_keep(seed, (uint32_t)r * (uint32_t)Hd + (uint32_t)(col + k), thresh) ? d[k] * inv : 0.f;
                    const float xv = word[id * Hd + col + k] + pos[(long)xp * Hd + col + k] + type0[col + k];
                    xh[it][k] = (xv - mean) * rstd;
                    gy[it][k] = gamma[col + k] * d[k];
                    s1 += gy[it][k]; s2 += gy[it][k] * xh[it][k];
                    a_g[it][k] += d[k] * xh[it][k];
                    a_b[it][k] += d[k];
                }
            }
        }
        const float m1 = wave_sum(s1) / Hd, m2 = wave_sum(s2) / Hd;
#pragma unroll
        for (int it = 0; it < MAXC; ++it) {
            const int col = (it * 64 + lane) * 8;
            if (col < Hd) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float dx = rstd * (gy[it][k] - m1 - xh[it][k] * m2);
                    a_x[it][k] += dx;
                    atomicAdd(d_word + id * Hd + col + k, dx);
                }
            }
        }
    }
#pragma unroll
    for (int it = 0; it < MAXC; ++it) {
        const int col = (it * 64 + lane) * 8;
        if (col < Hd) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                red[(wave * 3 + 0) * Hd + col + k] = a_g[it][k];
                red[(wave * 3 + 1) * Hd + col + k] = a_b[it][k];
                red[(wave * 3 + 2) * Hd + col + k] = a_x[it][k];
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < Hd; c += 256) {
        float g = 0.f, bsum = 0.f, x = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { g += red[(w * 3 + 0) * Hd + c]; bsum += red[(w * 3 + 1) * Hd + c]; x += red[(w * 3 + 2) * Hd + c]; }
        atomicAdd(dgamma + c, g);
        atomicAdd(dbeta + c, bsum);
        atomicAdd(d_pos + (long)xp * Hd + c, x);
        atomicAdd(d_type0 + c, x);
    }
}

extern "C" int lav_text_embed_fwd(void* stream, int n, int X, int Hd, const int64_t* ids, const float* word, const float* pos,
                                  const float* type0, const float* gamma, const float* beta, float eps, float dropout_p,
                                  uint32_t seed, void* out, float* mean, float* rstd) {
    LAV_REQUIRE(n > 0 && X > 0 && Hd % 8 == 0 && Hd <= 1024, "lav_text_embed_fwd: bad shape");
    LAV_REQUIRE(ids && word && pos && type0 && gamma && beta && out && mean && rstd, "lav_text_embed_fwd: null pointer");
    long rows = (long)n * X;
    hipLaunchKernelGGL(text_embed_fwd_kernel<2>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, n, X, Hd, ids, word,
                       pos, type0, gamma, beta, eps, dropout_p, seed, lav_drop_thresh(dropout_p), (bf16_t*)out, mean, rstd, 0,
                       (const bf16_t*)nullptr, 0L);
    return lav_check_launch("lav_text_embed_fwd");
}

extern "C" int lav_text_embed_pre_fwd(void* stream, int n, int Lp, int X, int Hd, const int64_t* ids, const float* word, const float* pos,
                                      const float* type0, const float* gamma, const float* beta, float eps, float dropout_p, uint32_t seed,
                                      const void* pre, long pre_stride, void* out, float* mean, float* rstd) {
    LAV_REQUIRE(n > 0 && X > 0 && Lp >= 0 && Hd % 8 == 0 && Hd <= 1024, "lav_text_embed_pre_fwd: bad shape n=%d Lp=%d X=%d Hd=%d", n, Lp, X, Hd);
    LAV_REQUIRE(ids && word && pos && type0 && gamma && beta && out && mean && rstd && (Lp == 0 || pre), "lav_text_embed_pre_fwd: null pointer");
    LAV_REQUIRE(pre_stride == 0 || pre_stride == (long)Lp * Hd, "lav_text_embed_pre_fwd: pre_stride must be 0 (one broadcast block) or Lp * Hd (a block per text), got %ld", pre_stride);
    LAV_REQUIRE(Lp == 0 || ((uintptr_t)pre & 15) == 0, "lav_text_embed_pre_fwd: pre must be 16-byte aligned");
    long rows = (long)n * (X + Lp);
    hipLaunchKernelGGL(text_embed_fwd_kernel<2>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, n, X, Hd, ids, word,
                       pos, type0, gamma, beta, eps, dropout_p, seed, lav_drop_thresh(dropout_p), (bf16_t*)out, mean, rstd, Lp,
                       (const bf16_t*)pre, pre_stride);
    return lav_check_launch("lav_text_embed_pre_fwd");
}

extern "C" int lav_text_embed_bwd(void* stream, int n, int X, int Hd, const int64_t* ids, const void* dout, const float* word,
                                  const float* pos, const float* type0, const float* gamma, const float* mean, const float* rstd,
                                  float dropout_p, uint32_t seed, float* d_word, float* d_pos, float* d_type0, float* dgamma,
                                  float* dbeta) {
    LAV_REQUIRE(n > 0 && X > 0 && Hd % 8 == 0 && Hd <= 1024, "lav_text_embed_bwd: bad shape");
    LAV_REQUIRE(ids && dout && d_word && d_pos && d_type0 && dgamma && dbeta, "lav_text_embed_bwd: null pointer");
    long rows = (long)n * X;
    const int groups = n >= 32 ? 8 : (n >= 8 ? 2 : 1);
    (void)rows;
    hipLaunchKernelGGL(text_embed_bwd_kernel<2>, dim3(X, groups), dim3(256), (size_t)12 * Hd * sizeof(float), (hipStream_t)stream, n, X, Hd, ids,
                       (const bf16_t*)dout, word, pos, type0, gamma, mean, rstd, dropout_p, seed, lav_drop_thresh(dropout_p), d_word,
                       d_pos, d_type0, dgamma, dbeta, 0, 0L, (void*)nullptr, 0, (float*)nullptr);
    return lav_check_launch("lav_text_embed_bwd");
}

extern "C" int lav_text_embed_pre_bwd(void* stream, int n, int Lp, int X, int Hd, const int64_t* ids, const void* dout, const float* word,
                                      const float* pos, const float* type0, const float* gamma, const float* mean, const float* rstd,
                                      float dropout_p, uint32_t seed, float* d_word, float* d_pos, float* d_type0, float* dgamma,
                                      float* dbeta, long pre_stride, void* d_pre, int d_pre_mode) {
    LAV_REQUIRE(n > 0 && X > 0 && Lp >= 0 && Hd % 8 == 0 && Hd <= 1024, "lav_text_embed_pre_bwd: bad shape n=%d Lp=%d X=%d Hd=%d", n, Lp, X, Hd);
    LAV_REQUIRE(ids && dout && d_word && d_pos && d_type0 && dgamma && dbeta && (Lp == 0 || d_pre), "lav_text_embed_pre_bwd: null pointer");
    LAV_REQUIRE(pre_stride == 0 || pre_stride == (long)Lp * Hd, "lav_text_embed_pre_bwd: pre_stride must be 0 or Lp * Hd, got %ld", pre_stride);
    LAV_REQUIRE(d_pre_mode == 0 || d_pre_mode == 1, "lav_text_embed_pre_bwd: d_pre_mode must be 0 (fp32 accumulate) or 1 (bf16 rows)");
    LAV_REQUIRE(pre_stride == 0 || d_pre_mode == 1, "lav_text_embed_pre_bwd: a pre-text block per text (pre_stride = Lp * Hd) returns bf16 rows (d_pre_mode 1)");
    const int groups = n >= 32 ? 8 : (n >= 8 ? 2 : 1);
    float* part = nullptr;
    const bool finish = Lp > 0 && pre_stride == 0 && groups > 1;
    if (finish) {
        size_t cap = 0;
        part = (float*)lav_ws_get(stream, LAV_WS_LN_PARTIALS, (size_t)groups * Lp * Hd * sizeof(float), &cap);
        if (!part) return LAV_E_WORKSPACE;
    }
    hipLaunchKernelGGL(text_embed_bwd_kernel<2>, dim3(X + Lp, groups), dim3(256), (size_t)12 * Hd * sizeof(float), (hipStream_t)stream, n, X,
                       Hd, ids, (const bf16_t*)dout, word, pos, type0, gamma, mean, rstd, dropout_p, seed, lav_drop_thresh(dropout_p), d_word,
                       d_pos, d_type0, dgamma, dbeta, Lp, pre_stride, d_pre, d_pre_mode, part);
    if (int rc = lav_check_launch("lav_text_embed_pre_bwd")) return rc;
    if (!finish) return LAV_OK;
    hipLaunchKernelGGL(text_pre_grad_finish_kernel, dim3(Lp), dim3(256), 0, (hipStream_t)stream, groups, Lp, Hd, (const float*)part, d_pre,
                       d_pre_mode);
    return lav_check_launch("lav_text_embed_pre_bwd (finish)");
}

// ---- row gather / gather-sum -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_kernel(int n_rows, int C, const bf16_t* src, long lds_, const int32_t* src_row,
                                                         bf16_t* dst, long ldd) {
    const int cpr = C / 8;
    const long total = (long)n_rows * cpr;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = idx % cpr; const long r = idx / cpr;
        const int sr = src_row[r];
        uint4 v = make_uint4(0, 0, 0, 0);
        if (sr >= 0) v = *(const uint4*)(src + (long)sr * lds_ + c * 8);
        *(uint4*)(dst + r * ldd + c * 8) = v;
    }
}

__global__ __launch_bounds__(256) void gather_sum_rows_kernel(int n_out, int C, const bf16_t* src, long lds_, const int32_t* start,
                                                             const int32_t* list, bf16_t* out, long ldo) {
    const int cpr = C / 8;
    const long total = (long)n_out * cpr;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = idx % cpr; const long r = idx / cpr;
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = start[r]; k < start[r + 1]; ++k) {
            float v[8];
            uint4 u = *(const uint4*)(src + (long)list[k] * lds_ + c * 8);
            unpack8(u, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += v[e];
        }
        *(uint4*)(out + r * ldo + c * 8) = pack8(acc);
    }
}

extern "C" int lav_gather_rows(void* stream, int n_rows, int C, const void* src, long lds_, const int32_t* src_row, void* dst,
                               long ldd) {
    LAV_REQUIRE(n_rows > 0 && C > 0 && C % 8 == 0 && src && src_row && dst, "lav_gather_rows: bad arguments");
    long total = (long)n_rows * (C / 8);
    int grid = (int)((total + 255) / 256 > 65535 ? 65535 : (total + 255) / 256);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n_rows, C, (const bf16_t*)src, lds_, src_row,
                       (bf16_t*)dst, ldd);
    return lav_check_launch("lav_gather_rows");
}

extern "C" int lav_gather_sum_rows(void* stream, int n_out, int C, const void* src, long lds_, const int32_t* start,
                                   const int32_t* list, void* out, long ldo) {
    LAV_REQUIRE(n_out > 0 && C > 0 && C % 8 == 0 && src && start && list && out, "lav_gather_sum_rows: bad arguments");
    long total = (long)n_out * (C / 8);
    int grid = (int)((total + 255) / 256 > 65535 ? 65535 : (total + 255) / 256);
    hipLaunchKernelGGL(gather_sum_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n_out, C, (const bf16_t*)src, lds_, start,
                       list, (bf16_t*)out, ldo);
    return lav_check_launch("lav_gather_sum_rows");
}

// ---- key mask of a pair list: out[k][c] = c < Lv ? mask_img[vi[k]][c] : mask_txt[ti[k]][c - Lv]  (int32, what the sequence-attention kernels read) ----
// vi / ti are NOT bounds-checked here: the caller validates them against B and nt (lavender_amd/hip.py pair_key_mask).  A mask with no columns is
// never read and may be null (torch hands out a null pointer for an empty tensor).
__global__ __launch_bounds__(256) void pair_key_mask_kernel(int n, int Lv, int X, const int64_t* __restrict__ mimg, const int64_t* __restrict__ mtxt,
                                                           const int32_t* __restrict__ vi, const int32_t* __restrict__ ti, int32_t* __restrict__ out) {
    const int L = Lv + X;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)n * L) return;
    const int k = (int)(idx / L), c = (int)(idx - (long)k * L);
    const int64_t m = c < Lv ? mimg[(long)vi[k] * Lv + c] : mtxt[(long)ti[k] * X + (c - Lv)];
    out[idx] = (int32_t)m;
}

extern "C" int lav_pair_key_mask(void* stream, int n, int Lv, int X, const int64_t* mask_img, const int64_t* mask_txt, const int32_t* vi,
                                 const int32_t* ti, int32_t* out) {
    LAV_REQUIRE(n > 0 && Lv >= 0 && X >= 0 && Lv + X > 0 && (Lv == 0 || mask_img) && (X == 0 || mask_txt) && vi && ti && out, "lav_pair_key_mask: bad arguments n=%d Lv=%d X=%d", n, Lv, X);
    const long tot = (long)n * (Lv + X);
    hipLaunchKernelGGL(pair_key_mask_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, Lv, X, mask_img, mask_txt, vi, ti, out);
    return lav_check_launch("lav_pair_key_mask");
}
