// Flash-style attention for gfx950, forward + backward, for both attention shapes on the LAVENDER path:
//   window mode   (Swin):  problems = (window, head), N = wd*wh*ww tokens (245 / 196 / 49 / 720), head_dim 32.
//                 Cyclic shift, window partition/reverse are index math on the un-rolled token tensor; the
//                 relative-position bias is gathered from an LDS copy of this head's table column with
//                 index = code(q) - code(k) + const; the shift mask is region(q) != region(k) ? -100 : 0.
//   sequence mode (fusion BERT): problems = (sequence, head), N = L (282 / 276 / 757), head_dim 64, key mask,
//                 attention-probability dropout regenerated from a counter hash.
// Score tiles are 32x32 MFMA tiles computed transposed (keys x queries) so each lane owns ONE query column:
// softmax statistics are lane-local (plus one cross-half shuffle) and the probability tile feeds the P.V MFMA
// as a B operand straight from registers.  K sits in LDS swizzled for ds_read_b128 A-fragments; V sits
// row-major and is read with ds_read_b64_tr_b16 (hardware transpose) as the A operand of O^T = V^T P^T.
#include "attn_common.h"
#include <stdlib.h>

#define LOG2E 1.4426950408889634f

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// CAUSAL (sequence mode): the seq2seq mask of LAVENDER_Base.get_attn_mask (model.py:208-218): keys below causal_from (the video
// / pre-text prefix) follow the key mask for EVERY query; keys at or above it (the text) are visible only to text queries at
// or after them (lower-triangular block); prefix queries see no text key.
template <int HD, int MODE, int KT, int KL, bool CAUSAL = false>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                                  // KL x HD bf16, K-type swizzle
    char* Vs = Ks + KL * HD * 2;                      // KL x HD bf16, V-type layout
    int* kinfo = (int*)(Vs + KL * HD * 2);            // KL x int32: window: code | region << 16; sequence: additive mask bits
    float* tbl = (float*)(kinfo + KL);                // window mode: this head's bias-table column

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, hi = lane >> 5;
    const int prob = blockIdx.x / a.d.heads, head = blockIdx.x % a.d.heads;
    const int N = a.N, C = a.C, ld = 3 * C;
    const bf16_t* qkv = a.qkv;

    if (MODE == 0) {
        for (int r = tid; r < a.tbl_rows; r += 256) tbl[r] = a.d.bias_table[(long)r * a.d.heads + head];
    }

    for (int rr = 0; rr < a.R; ++rr) {
        const int qt = (blockIdx.y * a.R + rr) * 4 + wave;
        const bool q_active = qt < a.nqt;              // wave-uniform
        const int q = qt * 32 + j;
        const bool q_ok = q_active && q < N;
        int q_row = 0, q_code = 0, q_reg = 0;
        if (q_ok) {
            if (MODE == 0) { TokInfo t = win_token(a, prob, q); q_row = t.row; q_code = t.code; q_reg = t.region; }
            else q_row = prob * N + q;
        }
        bf16x8 qf[HD / 16];
#pragma unroll
        for (int ks = 0; ks < HD / 16; ++ks) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (q_ok) v = *(const uint4*)(qkv + (long)q_row * ld + head * HD + ks * 16 + 8 * hi);
            qf[ks] = as_bf16x8(v);
        }
        f32x16 o[HD / 32];
#pragma unroll
        for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
        float m_run = -INFINITY, l_run = 0.f;

        for (int kc0 = 0; kc0 < N; kc0 += KL) {
            // ---- stage K / V rows [kc0, kc0+KL) and the per-key info ----------------------------------
            if (rr > 0 || kc0 > 0) __syncthreads();
            if (rr == 0 || N > KL) {
                constexpr int CPR = HD / 8;            // 16-byte chunks per row
                for (int c = tid; c < KL * CPR; c += 256) {
                    const int row = c / CPR, slot = c % CPR;
                    const int key = kc0 + row;
                    uint4 kv = make_uint4(0, 0, 0, 0), vv = kv;
                    if (key < N) {
                        int krow;
                        if (MODE == 0) krow = win_token(a, prob, key).row; else krow = prob * N + key;
                        const bf16_t* p = qkv + (long)krow * ld + head * HD + slot * 8;
                        kv = *(const uint4*)(p + C);
                        vv = *(const uint4*)(p + 2 * C);
                    }
                    *(uint4*)(Ks + krow_off<HD>(row, slot)) = kv;
                    *(uint4*)(Vs + vrow_off<HD>(row, slot)) = vv;
                }
                for (int row = tid; row < KL; row += 256) {
                    const int key = kc0 + row;
                    int info = 0;
                    if (MODE == 0) {
                        if (key < N) { TokInfo t = win_token(a, prob, key); info = t.code | (t.region << 16); }
                    } else {
                        float add = 0.f;
                        if (key >= N || (a.d.key_mask && a.d.key_mask[(long)prob * N + key] == 0)) add = -INFINITY;
                        info = __float_as_int(add);
                    }
                    kinfo[row] = info;
                }
            }
            __syncthreads();
            if (!q_active) continue;

            const int kl_keys = min(KL, N - kc0);
            for (int sc0 = 0; sc0 < kl_keys; sc0 += 32 * KT) {
                // ---- S^T tiles: keys x queries -----------------------------------------------------
                f32x16 s[KT];
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
                    const int k0 = sc0 + kt * 32;
                    if (k0 >= kl_keys) continue;
#pragma unroll
                    for (int ks = 0; ks < HD / 16; ++ks) {
                        bf16x8 kf = *(const bf16x8*)(Ks + krow_off<HD>(k0 + j, ks * 2 + hi));
                        s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[kt], 0, 0, 0);
                    }
                }
                // ---- scale + bias + mask, running max ---------------------------------------------
                float mx = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    const int k0 = sc0 + kt * 32;
                    if (k0 >= kl_keys) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) s[kt][r] = -INFINITY;
                        continue;
                    }
                    if constexpr (MODE == 1) {
                        // sequence mode: the additive key mask already holds -inf for masked / out-of-range keys
                        const float sc = a.d.scale * LOG2E;
#pragma unroll
                        for (int r4 = 0; r4 < 4; ++r4) {
                            const float4 ad = *(const float4*)((const float*)kinfo + k0 + 8 * r4 + 4 * hi);
                            const float ads[4] = {ad.x, ad.y, ad.z, ad.w};
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                float v = fmaf(s[kt][r4 * 4 + e], sc, ads[e]);
                                if (CAUSAL) {
                                    const int kk = kc0 + k0 + 8 * r4 + 4 * hi + e;
                                    if (kk >= a.d.causal_from && (q < a.d.causal_from || kk > q)) v = -INFINITY;
                                }
                                s[kt][r4 * 4 + e] = v;
                                mx = fmaxf(mx, v);
                            }
                        }
                        continue;
                    }
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const int kb = k0 + 8 * r4 + 4 * hi;           // 4 consecutive keys
                        const int4 inf = *(const int4*)(kinfo + kb);
                        const int infs[4] = {inf.x, inf.y, inf.z, inf.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float v = s[kt][r4 * 4 + e] * (a.d.scale * LOG2E);          // exp2 domain
                            if (MODE == 0) {
                                const int kcode = infs[e] & 0xffff, kreg = infs[e] >> 16;
                                v += tbl[q_code - kcode + a.tbl_const] * LOG2E;
                                if (kreg != q_reg) v += -100.0f * LOG2E;
                            } else {
                                v += __int_as_float(infs[e]);
                            }
                            if (kc0 + kb + e >= N) v = -INFINITY;
                            s[kt][r4 * 4 + e] = v;
                            mx = fmaxf(mx, v);
                        }
                    }
                }
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float m_new = fmaxf(m_run, mx);
                const float m_use = m_new == -INFINITY ? 0.f : m_new;
                const float alpha = fast_exp2(m_run - m_use);         // m_run = -inf -> 0
                l_run *= alpha;
#pragma unroll
                for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
                m_run = m_new;
                // ---- P = exp(S - m), O^T += V^T P^T -------------------------------------------------
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    const int k0 = sc0 + kt * 32;
                    if (k0 >= kl_keys) continue;
                    float p[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) { p[r] = fast_exp2(s[kt][r] - m_use); l_run += p[r]; }
                    if (MODE == 1 && a.d.dropout_p > 0.f) {
                        // one 64-bit hash per group of FOUR keys (this lane holds keys kb..kb+3 of each group of 8): index = (row, key >> 2)
                        const float inv = 1.f / (1.f - a.d.dropout_p);
                        const uint32_t pb = ((uint32_t)(prob * a.d.heads + head) * (uint32_t)N + (uint32_t)q) * (uint32_t)a.NH +
                                            (uint32_t)((kc0 + k0 + 4 * hi) >> 2);
#pragma unroll
                        for (int r4 = 0; r4 < 4; ++r4) {
                            const uint2 hq = lav_hash64(a.d.seed, pb + (uint32_t)(2 * r4));
#pragma unroll
                            for (int e2 = 0; e2 < 2; ++e2) {
                                const uint32_t h = e2 ? hq.y : hq.x;
                                const int r = r4 * 4 + 2 * e2;
                                p[r] = (h & 0xffffu) >= a.thresh16 ? p[r] * inv : 0.f;
                                p[r + 1] = (h >> 16) >= a.thresh16 ? p[r + 1] * inv : 0.f;
                            }
                        }
                    }
#pragma unroll
                    for (int sl = 0; sl < 2; ++sl) {
                        bf16x8 pf = pack_frag(p + 8 * sl);
#pragma unroll
                        for (int dt = 0; dt < HD / 32; ++dt) {
                            bf16x8 vf = tr_frag<HD>(Vs, k0 + 16 * sl, dt * 32, lane);
                            o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
                        }
                    }
                }
            }
        }
        if (!q_active) continue;
        // ---- epilogue: O = O^T / l ---------------------------------------------------------------
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        const float inv_l = l_tot > 0.f ? 1.f / l_tot : 0.f;
        if (q_ok) {
            bf16_t* op = a.o_w + (long)q_row * C + head * HD;
#pragma unroll
            for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int d = dt * 32 + 8 * r4 + 4 * hi;
                    uint2 w;
                    w.x = pack2(o[dt][r4 * 4 + 0] * inv_l, o[dt][r4 * 4 + 1] * inv_l);
                    w.y = pack2(o[dt][r4 * 4 + 2] * inv_l, o[dt][r4 * 4 + 3] * inv_l);
                    *(uint2*)(op + d) = w;
                }
            if (a.lse && hi == 0) a.lse[(long)blockIdx.x * a.Npad + q] = m_run + log2f(l_tot);   // log2 domain
        }
    }
}

// ------------------------------------------------------------------------------------------------
// backward, pass 1: dQ (+ relative-position-bias gradient).  Wave owns a 32-query tile, loops over keys.
//   S^T = K Q^T ; P^T = exp(S^T - lse) ; dP^T = V dO^T ; dS^T = P^T o (dP^T - delta) ; dQ^T = K^T dS^T * scale
// delta[q] = sum_d dO[q,d] O[q,d] is computed here and stored (fp32, lse layout, second half of the lse buffer).
// ------------------------------------------------------------------------------------------------
template <int HD, int MODE, int KL, bool CAUSAL = false>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(AttnArgs a, float* delta_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                                  // K-type (A operand of S^T)
    char* Kv = Ks + KL * HD * 2;                      // V-type copy of K (tr-read A operand of dQ^T)
    char* Vs = Kv + KL * HD * 2;                      // K-type V (A operand of dP^T)
    int* kinfo = (int*)(Vs + KL * HD * 2);
    float* tbl = (float*)(kinfo + KL);                // bias table column
    float* dtbl = tbl + a.tbl_rows;                   // its gradient (LDS accumulation, flushed with atomics)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, hi = lane >> 5;
    const int prob = blockIdx.x / a.d.heads, head = blockIdx.x % a.d.heads;
    const int N = a.N, C = a.C, ld = 3 * C;
    const bf16_t* qkv = a.qkv;

    if (MODE == 0) {
        for (int r = tid; r < a.tbl_rows; r += 256) { tbl[r] = a.d.bias_table[(long)r * a.d.heads + head]; dtbl[r] = 0.f; }
    }

    for (int rr = 0; rr < a.R; ++rr) {
        const int qt = (blockIdx.y * a.R + rr) * 4 + wave;
        const bool q_active = qt < a.nqt;
        const int q = qt * 32 + j;
        const bool q_ok = q_active && q < N;
        int q_row = 0, q_code = 0, q_reg = 0;
        if (q_ok) {
            if (MODE == 0) { TokInfo t = win_token(a, prob, q); q_row = t.row; q_code = t.code; q_reg = t.region; }
            else q_row = prob * N + q;
        }
        bf16x8 qf[HD / 16], dof[HD / 16];
        float dl = 0.f;
#pragma unroll
        for (int ks = 0; ks < HD / 16; ++ks) {
            uint4 v = make_uint4(0, 0, 0, 0), g = v, ov = v;
            if (q_ok) {
                v = *(const uint4*)(qkv + (long)q_row * ld + head * HD + ks * 16 + 8 * hi);
                g = *(const uint4*)(a.dout + (long)q_row * C + head * HD + ks * 16 + 8 * hi);
                ov = *(const uint4*)(a.out + (long)q_row * C + head * HD + ks * 16 + 8 * hi);
            }
            qf[ks] = as_bf16x8(v); dof[ks] = as_bf16x8(g);
            float gf[8], of[8];
            unpack8(g, gf); unpack8(ov, of);
#pragma unroll
            for (int e = 0; e < 8; ++e) dl += gf[e] * of[e];
        }
        dl += __shfl_xor(dl, 32, 64);
        const float lse = q_ok ? a.lse[(long)blockIdx.x * a.Npad + q] : 0.f;
        if (q_ok && hi == 0) delta_out[(long)blockIdx.x * a.Npad + q] = dl;

        f32x16 dq[HD / 32];
#pragma unroll
        for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;

        for (int kc0 = 0; kc0 < N; kc0 += KL) {
            if (rr > 0 || kc0 > 0) __syncthreads();
            if (rr == 0 || N > KL) {
                constexpr int CPR = HD / 8;
                for (int c = tid; c < KL * CPR; c += 256) {
                    const int row = c / CPR, slot = c % CPR;
                    const int key = kc0 + row;
                    uint4 kv = make_uint4(0, 0, 0, 0), vv = kv;
                    if (key < N) {
                        int krow;
                        if (MODE == 0) krow = win_token(a, prob, key).row; else krow = prob * N + key;
                        const bf16_t* p = qkv + (long)krow * ld + head * HD + slot * 8;
                        kv = *(const uint4*)(p + C);
                        vv = *(const uint4*)(p + 2 * C);
                    }
                    *(uint4*)(Ks + krow_off<HD>(row, slot)) = kv;
                    *(uint4*)(Kv + vrow_off<HD>(row, slot)) = kv;
                    *(uint4*)(Vs + krow_off<HD>(row, slot)) = vv;
                }
                for (int row = tid; row < KL; row += 256) {
                    const int key = kc0 + row;
                    int info = 0;
                    if (MODE == 0) {
                        if (key < N) { TokInfo t = win_token(a, prob, key); info = t.code | (t.region << 16); }
                    } else {
                        float add = 0.f;
                        if (key >= N || (a.d.key_mask && a.d.key_mask[(long)prob * N + key] == 0)) add = -INFINITY;
                        info = __float_as_int(add);
                    }
                    kinfo[row] = info;
                }
            }
            __syncthreads();
            if (!q_active) continue;
            const int kl_keys = min(KL, N - kc0);
            for (int k0 = 0; k0 < kl_keys; k0 += 32) {
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
                for (int ks = 0; ks < HD / 16; ++ks) {
                    bf16x8 kf = *(const bf16x8*)(Ks + krow_off<HD>(k0 + j, ks * 2 + hi));
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
                    bf16x8 vf = *(const bf16x8*)(Vs + krow_off<HD>(k0 + j, ks * 2 + hi));
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dof[ks], dp, 0, 0, 0);
                }
                float ds[16];
                const float inv = (MODE == 1 && a.d.dropout_p > 0.f) ? 1.f / (1.f - a.d.dropout_p) : 1.f;
                const uint32_t base = ((uint32_t)(prob * a.d.heads + head) * (uint32_t)N + (uint32_t)q) * (uint32_t)N + (uint32_t)kc0;
                if constexpr (MODE == 1) {
                    // lean sequence path: masks folded into the additive key term (-inf) and the row's lse (+inf for a padded
                    // query), one dropout hash per key pair
                    const float sc = a.d.scale * LOG2E;
                    const float lse_q = q_ok ? lse : INFINITY;
                    const uint32_t pb = ((uint32_t)(prob * a.d.heads + head) * (uint32_t)N + (uint32_t)q) * (uint32_t)a.NH +
                                        (uint32_t)((kc0 + k0 + 4 * hi) >> 2);
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const float4 ad = *(const float4*)((const float*)kinfo + k0 + 8 * r4 + 4 * hi);
                        const float ads[4] = {ad.x, ad.y, ad.z, ad.w};
                        const uint2 hq = lav_hash64(a.d.seed, pb + (uint32_t)(2 * r4));              // p = 0: thresh16 = 0 keeps everything
#pragma unroll
                        for (int e2 = 0; e2 < 2; ++e2) {
                            const uint32_t h = e2 ? hq.y : hq.x;
                            const float m0 = (h & 0xffffu) >= a.thresh16 ? inv : 0.f;
                            const float m1 = (h >> 16) >= a.thresh16 ? inv : 0.f;
                            const int r = r4 * 4 + 2 * e2;
                            float p0 = fast_exp2(fmaf(s[r], sc, ads[2 * e2]) - lse_q);
                            float p1 = fast_exp2(fmaf(s[r + 1], sc, ads[2 * e2 + 1]) - lse_q);
                            if (CAUSAL) {
                                const int kk = kc0 + k0 + 8 * r4 + 4 * hi + 2 * e2;
                                if (kk >= a.d.causal_from && (q < a.d.causal_from || kk > q)) p0 = 0.f;
                                if (kk + 1 >= a.d.causal_from && (q < a.d.causal_from || kk + 1 > q)) p1 = 0.f;
                            }
                            ds[r] = p0 * (dp[r] * m0 - dl);
                            ds[r + 1] = p1 * (dp[r + 1] * m1 - dl);
                        }
                    }
                } else
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int kb = k0 + 8 * r4 + 4 * hi;
                    const int4 inf = *(const int4*)(kinfo + kb);
                    const int infs[4] = {inf.x, inf.y, inf.z, inf.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = r4 * 4 + e;
                        float v = s[r] * (a.d.scale * LOG2E);
                        int bidx = 0;
                        if (MODE == 0) {
                            const int kcode = infs[e] & 0xffff, kreg = infs[e] >> 16;
                            bidx = q_code - kcode + a.tbl_const;
                            v += tbl[bidx] * LOG2E;
                            if (kreg != q_reg) v += -100.0f * LOG2E;
                        } else {
                            v += __int_as_float(infs[e]);
                        }
                        const bool valid = q_ok && (kc0 + kb + e < N);
                        float p = valid ? fast_exp2(v - lse) : 0.f;
                        float g = dp[r];
                        if (MODE == 1 && a.d.dropout_p > 0.f)
                            g = lav_keep(a.d.seed, base + (uint32_t)(kb + e), a.thresh) ? g * inv : 0.f;
                        const float dsv = p * (g - dl);
                        ds[r] = dsv;
                        if (MODE == 0 && valid) atomicAdd(&dtbl[bidx], dsv);
                    }
                }
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    bf16x8 dsf = pack_frag(ds + 8 * sl);
#pragma unroll
                    for (int dt = 0; dt < HD / 32; ++dt) {
                        bf16x8 kt_ = tr_frag<HD>(Kv, k0 + 16 * sl, dt * 32, lane);
                        dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt_, dsf, dq[dt], 0, 0, 0);
                    }
                }
            }
        }
        if (q_ok) {
            bf16_t* op = a.dqkv + (long)q_row * ld + head * HD;
#pragma unroll
            for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int d = dt * 32 + 8 * r4 + 4 * hi;
                    uint2 w;
                    w.x = pack2(dq[dt][r4 * 4 + 0] * a.d.scale, dq[dt][r4 * 4 + 1] * a.d.scale);
                    w.y = pack2(dq[dt][r4 * 4 + 2] * a.d.scale, dq[dt][r4 * 4 + 3] * a.d.scale);
                    *(uint2*)(op + d) = w;
                }
        }
    }
    if (MODE == 0 && a.dbias) {
        __syncthreads();
        for (int r = tid; r < a.tbl_rows; r += 256) {
            const float v = dtbl[r];
            if (v != 0.f) atomicAdd(a.dbias + (long)r * a.d.heads + head, v);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// backward, pass 2: dK, dV.  Wave owns a 32-key tile, loops over queries staged in LDS.
//   S = Q K^T (queries x keys) ; P = exp(S - lse[q]) ; dP = dO V^T ; dS = P o (dP - delta[q])
//   dV^T = dO^T P~   (P~ = dropout(P)) ;  dK^T = Q^T dS * scale
// ------------------------------------------------------------------------------------------------
template <int HD, int MODE, int QL, bool CAUSAL = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(AttnArgs a, const float* delta_in) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qs = smem;                                  // K-type: A operand of S
    char* Qv = Qs + QL * HD * 2;                      // V-type: tr-read A operand of dK^T
    char* Gs = Qv + QL * HD * 2;                      // dO, K-type: A operand of dP
    char* Gv = Gs + QL * HD * 2;                      // dO, V-type: tr-read A operand of dV^T
    int* qinfo = (int*)(Gv + QL * HD * 2);            // per query: code | region << 16
    float* qlse = (float*)(qinfo + QL);
    float* qdl = qlse + QL;
    float* tbl = qdl + QL;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, hi = lane >> 5;
    const int prob = blockIdx.x / a.d.heads, head = blockIdx.x % a.d.heads;
    const int N = a.N, C = a.C, ld = 3 * C;
    const bf16_t* qkv = a.qkv;

    if (MODE == 0) {
        for (int r = tid; r < a.tbl_rows; r += 256) tbl[r] = a.d.bias_table[(long)r * a.d.heads + head];
    }

    for (int rr = 0; rr < a.R; ++rr) {
        const int kt = (blockIdx.y * a.R + rr) * 4 + wave;
        const bool k_active = kt < a.nqt;
        const int key = kt * 32 + j;
        const bool k_ok = k_active && key < N;
        int k_row = 0, k_code = 0, k_reg = 0;
        float k_add = 0.f;
        if (k_ok) {
            if (MODE == 0) { TokInfo t = win_token(a, prob, key); k_row = t.row; k_code = t.code; k_reg = t.region; }
            else {
                k_row = prob * N + key;
                if (a.d.key_mask && a.d.key_mask[(long)prob * N + key] == 0) k_add = -INFINITY;
            }
        }
        if (MODE == 1 && !k_ok) k_add = -INFINITY;          // padded key lanes: P = 0 without a per-element validity test
        bf16x8 kf[HD / 16], vf[HD / 16];
#pragma unroll
        for (int ks = 0; ks < HD / 16; ++ks) {
            uint4 kv = make_uint4(0, 0, 0, 0), vv = kv;
            if (k_ok) {
                const bf16_t* p = qkv + (long)k_row * ld + head * HD + ks * 16 + 8 * hi;
                kv = *(const uint4*)(p + C);
                vv = *(const uint4*)(p + 2 * C);
            }
            kf[ks] = as_bf16x8(kv); vf[ks] = as_bf16x8(vv);
        }
        f32x16 dk[HD / 32], dv[HD / 32];
#pragma unroll
        for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { dk[dt][r] = 0.f; dv[dt][r] = 0.f; }

        for (int qc0 = 0; qc0 < N; qc0 += QL) {
            if (rr > 0 || qc0 > 0) __syncthreads();
            if (rr == 0 || N > QL) {
                constexpr int CPR = HD / 8;
                for (int c = tid; c < QL * CPR; c += 256) {
                    const int row = c / CPR, slot = c % CPR;
                    const int q = qc0 + row;
                    uint4 qv = make_uint4(0, 0, 0, 0), gv = qv;
                    if (q < N) {
                        int qrow;
                        if (MODE == 0) qrow = win_token(a, prob, q).row; else qrow = prob * N + q;
                        qv = *(const uint4*)(qkv + (long)qrow * ld + head * HD + slot * 8);
                        gv = *(const uint4*)(a.dout + (long)qrow * C + head * HD + slot * 8);
                    }
                    *(uint4*)(Qs + krow_off<HD>(row, slot)) = qv;
                    *(uint4*)(Qv + vrow_off<HD>(row, slot)) = qv;
                    *(uint4*)(Gs + krow_off<HD>(row, slot)) = gv;
                    *(uint4*)(Gv + vrow_off<HD>(row, slot)) = gv;
                }
                for (int row = tid; row < QL; row += 256) {
                    const int q = qc0 + row;
                    int info = 0; float l = 0.f, dl = 0.f;
                    if (q < N) {
                        if (MODE == 0) { TokInfo t = win_token(a, prob, q); info = t.code | (t.region << 16); }
                        l = a.lse[(long)blockIdx.x * a.Npad + q];
                        dl = delta_in[(long)blockIdx.x * a.Npad + q];
                    } else if (MODE == 1) {
                        l = INFINITY;                           // padded query rows: P = exp2(v - inf) = 0
                    }
                    qinfo[row] = info; qlse[row] = l; qdl[row] = dl;
                }
            }
            __syncthreads();
            if (!k_active) continue;
            const int ql = min(QL, N - qc0);
            for (int q0 = 0; q0 < ql; q0 += 32) {
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
                for (int ks = 0; ks < HD / 16; ++ks) {
                    bf16x8 qa = *(const bf16x8*)(Qs + krow_off<HD>(q0 + j, ks * 2 + hi));
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], s, 0, 0, 0);
                    bf16x8 ga = *(const bf16x8*)(Gs + krow_off<HD>(q0 + j, ks * 2 + hi));
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga, vf[ks], dp, 0, 0, 0);
                }
                float pd[16], ds[16];
                const float inv = (MODE == 1 && a.d.dropout_p > 0.f) ? 1.f / (1.f - a.d.dropout_p) : 1.f;
                if constexpr (MODE == 1) {
                    // lean sequence path (see the dQ pass); a lane holds ONE key here, so the group hash is indexed by
                    // (query row, key >> 2) and this lane takes the 16-bit field selected by key & 3
                    const float sc = a.d.scale * LOG2E;
                    const uint32_t nh = (uint32_t)a.NH;
                    const uint32_t rb0 = ((uint32_t)(prob * a.d.heads + head) * (uint32_t)N + (uint32_t)(qc0 + q0 + 4 * hi)) * nh + (uint32_t)(key >> 2);
                    const uint32_t sh = (uint32_t)(key & 1) * 16u;
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const int qb = q0 + 8 * r4 + 4 * hi;
                        const float4 l4 = *(const float4*)(qlse + qb);
                        const float4 d4 = *(const float4*)(qdl + qb);
                        const float ls[4] = {l4.x, l4.y, l4.z, l4.w};
                        const float dls[4] = {d4.x, d4.y, d4.z, d4.w};
                        const uint32_t rb = rb0 + (uint32_t)(8 * r4) * nh;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int r = r4 * 4 + e;
                            float p = fast_exp2(fmaf(s[r], sc, k_add) - ls[e]);
                            if (CAUSAL) {
                                const int qq = qc0 + qb + e;
                                if (key >= a.d.causal_from && (qq < a.d.causal_from || key > qq)) p = 0.f;
                            }
                            const uint2 hq = lav_hash64(a.d.seed, rb + (uint32_t)e * nh);     // p = 0: thresh16 = 0 keeps everything
                            const uint32_t h = (key & 2) ? hq.y : hq.x;
                            const float m = ((h >> sh) & 0xffffu) >= a.thresh16 ? inv : 0.f;
                            pd[r] = p * m;
                            ds[r] = p * (dp[r] * m - dls[e]);
                        }
                    }
                } else
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int qb = q0 + 8 * r4 + 4 * hi;
                    const int4 inf = *(const int4*)(qinfo + qb);
                    const float4 l4 = *(const float4*)(qlse + qb);
                    const float4 d4 = *(const float4*)(qdl + qb);
                    const int infs[4] = {inf.x, inf.y, inf.z, inf.w};
                    const float ls[4] = {l4.x, l4.y, l4.z, l4.w};
                    const float dls[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = r4 * 4 + e;
                        const int q = qc0 + qb + e;
                        float v = s[r] * (a.d.scale * LOG2E);
                        if (MODE == 0) {
                            const int qcode = infs[e] & 0xffff, qreg = infs[e] >> 16;
                            v += tbl[qcode - k_code + a.tbl_const] * LOG2E;
                            if (qreg != k_reg) v += -100.0f * LOG2E;
                        } else {
                            v += k_add;
                        }
                        const bool valid = k_ok && q < N;
                        const float p = valid ? fast_exp2(v - ls[e]) : 0.f;
                        float g = dp[r], pdrop = p;
                        if (MODE == 1 && a.d.dropout_p > 0.f) {
                            const uint32_t idx = ((uint32_t)(prob * a.d.heads + head) * (uint32_t)N + (uint32_t)q) * (uint32_t)N + (uint32_t)key;
                            const bool keep = lav_keep(a.d.seed, idx, a.thresh);
                            g = keep ? g * inv : 0.f;
                            pdrop = keep ? p * inv : 0.f;
                        }
                        pd[r] = pdrop;
                        ds[r] = p * (g - dls[e]);
                    }
                }
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    bf16x8 pf = pack_frag(pd + 8 * sl), dsf = pack_frag(ds + 8 * sl);
#pragma unroll
                    for (int dt = 0; dt < HD / 32; ++dt) {
                        bf16x8 gt = tr_frag<HD>(Gv, q0 + 16 * sl, dt * 32, lane);
                        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gt, pf, dv[dt], 0, 0, 0);
                        bf16x8 qt_ = tr_frag<HD>(Qv, q0 + 16 * sl, dt * 32, lane);
                        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qt_, dsf, dk[dt], 0, 0, 0);
                    }
                }
            }
        }
        if (k_ok) {
            bf16_t* op = a.dqkv + (long)k_row * ld + head * HD;
#pragma unroll
            for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int d = dt * 32 + 8 * r4 + 4 * hi;
                    uint2 w;
                    w.x = pack2(dk[dt][r4 * 4 + 0] * a.d.scale, dk[dt][r4 * 4 + 1] * a.d.scale);
                    w.y = pack2(dk[dt][r4 * 4 + 2] * a.d.scale, dk[dt][r4 * 4 + 3] * a.d.scale);
                    *(uint2*)(op + C + d) = w;
                    w.x = pack2(dv[dt][r4 * 4 + 0], dv[dt][r4 * 4 + 1]);
                    w.y = pack2(dv[dt][r4 * 4 + 2], dv[dt][r4 * 4 + 3]);
                    *(uint2*)(op + 2 * C + d) = w;
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
int attn_setup(const lav_attn_desc* d, AttnArgs& a, int& problems) {
    LAV_REQUIRE(d, "attention: null descriptor");
    memset(&a, 0, sizeof(a));
    a.d = *d;
    LAV_REQUIRE(d->heads > 0, "attention: heads=%d", d->heads);
    a.C = d->heads * d->head_dim;
    if (d->mode == 0) {
        LAV_REQUIRE(d->head_dim == 32, "attention(window): head_dim must be 32 (got %d)", d->head_dim);
        LAV_REQUIRE(d->wd > 0 && d->wh > 0 && d->ww > 0, "attention(window): bad window");
        LAV_REQUIRE(d->D % d->wd == 0 && d->H % d->wh == 0 && d->W % d->ww == 0,
                    "attention(window): token grid (%d,%d,%d) is not a multiple of the window (%d,%d,%d); the zero-pad "
                    "branch of video_swin.py:211-215 is not supported", d->D, d->H, d->W, d->wd, d->wh, d->ww);
        LAV_REQUIRE(d->sd < d->wd && d->sh < d->wh && d->sw < d->ww && d->sd >= 0 && d->sh >= 0 && d->sw >= 0, "attention(window): bad shift");
        LAV_REQUIRE(d->wd <= d->cfg_wd && d->wh <= d->cfg_wh && d->ww <= d->cfg_ww, "attention(window): window exceeds configured window");
        LAV_REQUIRE(d->bias_table, "attention(window): null bias table");
        a.N = d->wd * d->wh * d->ww;
        a.nWd = d->D / d->wd; a.nWh = d->H / d->wh; a.nWw = d->W / d->ww;
        problems = d->B * a.nWd * a.nWh * a.nWw;
        a.cstride_h = 2 * d->cfg_ww - 1;
        a.cstride_d = (2 * d->cfg_wh - 1) * a.cstride_h;
        a.tbl_rows = (2 * d->cfg_wd - 1) * a.cstride_d;
        a.tbl_const = (d->cfg_wd - 1) * a.cstride_d + (d->cfg_wh - 1) * a.cstride_h + (d->cfg_ww - 1);
        LAV_REQUIRE(a.tbl_rows < 65536, "attention(window): bias table too large");
    } else {
        LAV_REQUIRE(d->head_dim == 64, "attention(sequence): head_dim must be 64 (got %d)", d->head_dim);
        LAV_REQUIRE(d->n_seq > 0 && d->L > 0, "attention(sequence): bad shape");
        LAV_REQUIRE(d->causal_from >= 0 && d->causal_from <= d->L, "attention(sequence): causal_from %d outside [0, L]", d->causal_from);
        a.N = d->L;
        problems = d->n_seq;
    }
    if (d->mode == 0) {
        a.nWs = a.nWd * a.nWh * a.nWw;
        a.tps = d->D * d->H * d->W;
        if (d->comb || d->combT) {
            LAV_REQUIRE(a.N <= 256, "attention(window): the persistent path needs N <= 256 (got %d)", a.N);
            LAV_REQUIRE(d->comb && d->combT && d->tok_table && d->win_type && d->type_region && d->n_types > 0,
                        "attention(window): comb/combT/tok_table/win_type/type_region must be given together");
        }
    }
    a.nqt = (a.N + 31) / 32;
    a.Npad = a.nqt * 32;
    a.thresh = lav_drop_thresh(d->dropout_p);
    a.thresh16 = lav_drop_thresh16(d->dropout_p);
    a.NH = (a.N + 3) / 4;
    return LAV_OK;
}

extern "C" size_t lav_attention_lse_elems(const lav_attn_desc* d) {
    AttnArgs a; int problems = 0;
    if (attn_setup(d, a, problems)) return 0;
    return (size_t)2 * problems * d->heads * a.Npad;      // lse followed by delta (backward scratch)
}

// ---- switches: read from the environment once, when the library is loaded; lav_winl_select changes the query parts at run time -----------------
static bool env_on(const char* v) { return v ? atoi(v) != 0 : true; }
static AttnSwitches attn_sw = {env_on(getenv("LAV_WINL")), env_on(getenv("LAV_SEQL")), 0};
// test hook: force the number of query parts per large-window problem (0 = by problem count, -1 = large windows on the generic kernels)
extern "C" int lav_winl_select(int parts) { const int old = attn_sw.winl_parts; attn_sw.winl_parts = parts; return old; }

// ---- route plan: pure, the CPU tests call it through lav_attention_plan -------------------------------------------------------------------
static WlTab wl_tab(const AttnArgs& a) {
    const lav_attn_desc& d = a.d;
    const int i = a.N - 1;                                   // codes grow with the slot index: the last slot has the largest
    WlTab t;
    t.mc = (i / (d.cfg_wh * d.cfg_ww)) * a.cstride_d + ((i / d.cfg_ww) % d.cfg_wh) * a.cstride_h + (i % d.cfg_ww);
    t.lo = a.tbl_const - t.mc;
    t.n = 2 * t.mc + 1;
    return t;
}
// persistent kernels: batch slices per (head, window position[, key half]) so that ~256 workgroups exist
static int pick_bsplit(const AttnArgs& a, int per_pair) {
    const int base = a.d.heads * a.nWs * per_pair;
    int bs = (256 + base - 1) / base;
    if (bs > a.d.B) bs = a.d.B;
    if (bs < 1) bs = 1;
    return bs;
}

AttnPlan attn_plan(const AttnArgs& a, int problems, const AttnSwitches& sw) {
    const lav_attn_desc& d = a.d;
    AttnPlan p;
    memset(&p, 0, sizeof(p));
    p.NT = a.nqt;
    const unsigned nprob = (unsigned)(problems * d.heads);
    auto put = [&p](int pass, int kern, unsigned gx, unsigned gy, unsigned block, size_t lds, int split) {
        p.launch[pass][p.n[pass]++] = {kern, gx, gy, block, lds, split};
    };
    auto walk = [](unsigned items, unsigned cap) { return items < cap ? items : cap; };   // workgroups of a kernel that walks its items
    bool large = false, chunked = false;
    if (d.mode == 0 && !d.comb && sw.winl && sw.winl_parts >= 0 && a.N <= WL_ROWS) {
        p.tab = wl_tab(a);
        const double qkv_bytes = (double)d.B * a.tps * 3.0 * a.C * 2.0;             // DMA offsets are 32-bit
        large = qkv_bytes < 4.0e9 && p.tab.lo >= 0 && p.tab.lo + p.tab.n <= a.tbl_rows &&
                (size_t)p.tab.n * 4 + 2 * WL_IMG + 5 * WL_ROWS * 4 + 512 <= 160 * 1024 && (size_t)p.tab.n * 4 + WLB_MAIN + 384 * 4 + 512 <= 160 * 1024;
    }
    if (d.mode == 1 && a.N > SEQ3_ROWS)     // (32-bit DMA offsets per problem base are fine; keep the whole tensor below 4 GB anyway)
        chunked = sw.seql && a.N <= SEQL_ROWS && (double)d.n_seq * a.N * 3.0 * a.C * 2.0 < 4.0e9;

    if (d.mode == 0 && d.comb) {                             // N <= 256 with the fragment tables (attention_win.hip)
        p.route = AR_WIN_PERSISTENT; p.bias_split = true; p.delta_negated = true;
        const int bs = pick_bsplit(a, 1), bsb = pick_bsplit(a, 2);
        const unsigned grid = (unsigned)(d.heads * a.nWs * bs);
        put(AP_FWD, AK_WIN_FWD3, grid, 1, 512, 2 * 49152 + 1024, bs);
        put(AP_BWD, AK_WIN_BWD1, grid, 1, 512, 2 * (32768 + 1024) + 1024 + 8 * 6144 + 8 * 4096 + 1024 + 64, bs);
        put(AP_BIAS, AK_WIN_DBIAS3, (unsigned)(d.heads * a.nWs * bsb * 2), 1, 512, 128 * 257 * 4 + 1024, bsb);   // max(two operand buffers, the flush matrix) + token rows
    } else if (large) {                                      // N <= 768 without them (attention_winl.hip)
        p.route = AR_WIN_LARGE; p.bias_split = true;
        const int QS = sw.winl_parts > 0 ? sw.winl_parts : nprob >= 1024 ? 1 : 3;
        const unsigned grid = walk(nprob * QS, 256);
        const size_t lds = 2 * WL_IMG + 3 * WL_ROWS * 4 + (size_t)p.tab.n * 4;
        put(AP_FWD, AK_WINL_FWD, grid, 1, 512, lds, QS);
        put(AP_BWD, AK_WINL_DQ, grid, 1, 512, lds, QS);
        put(AP_BWD, AK_WINL_DKV, grid, 1, 512, lds + 2 * WL_ROWS * 4, QS);
        const int nqb = (a.nqt + 3) / 4, nkb = (a.nqt + 7) / 8, base = d.heads * nqb * nkb;
        int WS = (512 + base - 1) / base;
        if (WS > problems) WS = problems;
        if (WS < 1) WS = 1;
        put(AP_BIAS, AK_WINL_DBIAS, (unsigned)(base * WS), 1, 512, WLB_MAIN + 384 * 4 + (size_t)p.tab.n * 4, WS);
    } else if (chunked) {                                    // 288 < L <= 768 (attention_seq.hip, second half)
        p.route = AR_SEQ_CHUNKED;
        const int parts = (a.nqt + 7) / 8;
        const unsigned grid = walk(nprob * parts, 256);
        put(AP_FWD, AK_SEQL_FWD, grid, 1, 512, 2 * SEQL_BUF + SEQL_ROWS * 4, parts);
        put(AP_BWD, AK_SEQL_DQ, grid, 1, 512, 2 * SEQL_BUF + SEQL_ROWS * 4, parts);
        put(AP_BWD, AK_SEQL_DKV, grid, 1, 512, 2 * SEQL_BUF + SEQL_ROWS * 8, parts);
    } else if (d.mode == 1 && a.N <= SEQ3_ROWS) {            // L <= 288 (attention_seq.hip)
        p.route = AR_SEQ_ONE;
        const unsigned grid = walk(nprob, 512);
        put(AP_FWD, AK_SEQ_FWD3, grid, 1, 256, 2 * SEQ3_IMG + SEQ3_ROWS * 4, 0);
        put(AP_BWD, AK_SEQ_DQ3, grid, 1, 256, 2 * SEQ3_IMG + SEQ3_ROWS * 4, 0);
        put(AP_BWD, AK_SEQ_DKV3, grid, 1, 256, 2 * SEQ3_IMG + SEQ3_ROWS * 8, 0);
    } else {                                                 // the generic kernels of this file
        p.route = d.mode == 0 ? AR_GEN_WINDOW : AR_GEN_SEQ;
        const int qgroups = (a.nqt + 3) / 4;
        // a problem whose keys / queries fit one staged chunk takes one workgroup (R tile rounds per wave), else one per group of four tiles
        auto gen = [&](int pass, int kern, int chunk, size_t lds) {
            const bool one = a.N <= chunk;
            put(pass, kern, nprob, one ? 1 : qgroups, 256, lds, one ? qgroups : 1);
        };
        if (d.mode == 0) {
            gen(AP_FWD, AK_GEN_FWD, WIN_KL, (size_t)WIN_KL * 32 * 2 * 2 + WIN_KL * 4 + (size_t)a.tbl_rows * 4);
            gen(AP_BWD, AK_GEN_DQ, WIN_KL, (size_t)WIN_KL * 32 * 2 * 3 + WIN_KL * 4 + (size_t)a.tbl_rows * 8);
            gen(AP_BWD, AK_GEN_DKV, WIN_KL, (size_t)WIN_KL * 32 * 2 * 4 + WIN_KL * 12 + (size_t)a.tbl_rows * 4);
        } else {
            gen(AP_FWD, AK_GEN_FWD, SEQ_KL_FWD, (size_t)SEQ_KL_FWD * 64 * 2 * 2 + SEQ_KL_FWD * 4);
            gen(AP_BWD, AK_GEN_DQ, SEQ_KL, (size_t)SEQ_KL * 64 * 2 * 3 + SEQ_KL * 4);
            gen(AP_BWD, AK_GEN_DKV, SEQ_QL, (size_t)SEQ_QL * 64 * 2 * 4 + SEQ_QL * 12);
        }
    }
    // backward with the bias-table gradient: the split routes append their bias launch; the generic dQ kernel accumulates it itself (a.dbias)
    for (int i = 0; i < p.n[AP_BWD]; ++i) p.launch[AP_BWD_BIAS][p.n[AP_BWD_BIAS]++] = p.launch[AP_BWD][i];
    if (p.bias_split) p.launch[AP_BWD_BIAS][p.n[AP_BWD_BIAS]++] = p.launch[AP_BIAS][0];
    return p;
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------------
template <bool CAUSAL>
static void gen_seq_launch(hipStream_t s, const AttnArgs& a, const AttnLaunch& l, float* delta) {
    switch (l.kern) {
    case AK_GEN_FWD: attn_launch(attn_fwd_kernel<64, 1, 3, SEQ_KL_FWD, CAUSAL>, l, s, a); break;
    case AK_GEN_DQ: attn_launch(attn_bwd_dq_kernel<64, 1, SEQ_KL, CAUSAL>, l, s, a, delta); break;
    default: attn_launch(attn_bwd_dkv_kernel<64, 1, SEQ_QL, CAUSAL>, l, s, a, delta); break;
    }
}
static void gen_launch(hipStream_t s, AttnArgs& a, const AttnLaunch& l, float* delta) {
    a.R = l.split;
    if (a.d.mode == 1) { if (a.d.causal_from > 0) gen_seq_launch<true>(s, a, l, delta); else gen_seq_launch<false>(s, a, l, delta); return; }
    switch (l.kern) {
    case AK_GEN_FWD: attn_launch(attn_fwd_kernel<32, 0, 8, WIN_KL>, l, s, a); break;
    case AK_GEN_DQ: attn_launch(attn_bwd_dq_kernel<32, 0, WIN_KL>, l, s, a, delta); break;
    default: attn_launch(attn_bwd_dkv_kernel<32, 0, WIN_KL>, l, s, a, delta); break;
    }
}

// every launch of one pass of the plan, in order; delta = the scratch behind the lse
static int attn_run(void* stream, AttnArgs& a, int problems, const AttnPlan& p, int pass, const char* entry) {
    hipStream_t s = (hipStream_t)stream;
    float* delta = a.lse ? a.lse + (size_t)problems * a.d.heads * a.Npad : nullptr;
    for (int i = 0; i < p.n[pass]; ++i) {
        const AttnLaunch& l = p.launch[pass][i];
        if (l.kern <= AK_WIN_DBIAS3) win_launch(s, a, p, l, delta);
        else if (l.kern <= AK_WINL_DBIAS) winl_launch(s, a, p, l, delta);
        else if (l.kern <= AK_SEQL_DKV) seq_launch(s, a, p, l, delta);
        else gen_launch(s, a, l, delta);
    }
    return lav_check_launch(entry);
}

// ---- entries ----------------------------------------------------------------------------------------------------------------------------
// descriptor checks, the operand-layout checks every entry shares, and the plan
static int attn_prepare(const lav_attn_desc* d, const char* entry, AttnArgs& a, int& problems, AttnPlan& p) {
    if (int rc = attn_setup(d, a, problems)) return rc;
    LAV_REQUIRE(!d->qkv_headmajor || (d->mode == 0 && d->comb && d->head_dim == 32), "%s: qkv_headmajor needs window mode with the precomputed tables (N <= 256, head_dim 32)", entry);
    // head-major operand offsets are 32-bit byte offsets from the first token row: [q | k | v][head] planes of the WHOLE batch
    const long hm_bytes = 6L * d->heads * d->head_dim * d->B * d->D * d->H * d->W;
    LAV_REQUIRE(!d->qkv_headmajor || hm_bytes < (1L << 32), "%s: head-major qkv of %ld bytes exceeds the 4 GiB the window kernels address with 32-bit offsets", entry, hm_bytes);
    p = attn_plan(a, problems, attn_sw);
    return LAV_OK;
}

extern "C" int lav_attention_fwd(void* stream, const lav_attn_desc* d, const void* qkv, void* out, float* lse) {
    AttnArgs a; int problems = 0; AttnPlan p;
    LAV_REQUIRE(qkv && out, "lav_attention_fwd: null pointer");
    if (int rc = attn_prepare(d, "lav_attention_fwd", a, problems, p)) return rc;
    a.qkv = (const bf16_t*)qkv; a.o_w = (bf16_t*)out; a.lse = lse;
    return attn_run(stream, a, problems, p, AP_FWD, "lav_attention_fwd");
}

extern "C" int lav_attention_bwd(void* stream, const lav_attn_desc* d, const void* qkv, const void* out, const void* dout,
                                 const float* lse, void* dqkv, float* dbias_table) {
    AttnArgs a; int problems = 0; AttnPlan p;
    LAV_REQUIRE(qkv && out && dout && lse && dqkv, "lav_attention_bwd: null pointer");
    if (int rc = attn_prepare(d, "lav_attention_bwd", a, problems, p)) return rc;
    a.qkv = (const bf16_t*)qkv; a.out = (const bf16_t*)out; a.dout = (const bf16_t*)dout; a.lse = (float*)lse;
    a.dqkv = (bf16_t*)dqkv; a.dbias = dbias_table;
    return attn_run(stream, a, problems, p, dbias_table ? AP_BWD_BIAS : AP_BWD, "lav_attention_bwd");
}

// Bias-table gradient alone (window mode; persistent N <= 256 path or large-window path): needs the forward's lse and the delta scratch that
// lav_attention_bwd (called first, with dbias_table = NULL) left behind the lse in the same buffer -- NEGATED on the persistent route (win_bwd1
// writes -delta, the C operand of its dP MFMAs, and win_dbias3 reads it), +delta on the large-window one (winl_dq writes, winl_dbias reads):
// AttnPlan.delta_negated.  A parameter gradient: the engine issues it on the weight-gradient stream.
extern "C" int lav_attention_bwd_bias(void* stream, const lav_attn_desc* d, const void* qkv, const void* dout, const float* lse,
                                      float* dbias_table) {
    AttnArgs a; int problems = 0; AttnPlan p;
    LAV_REQUIRE(qkv && dout && lse && dbias_table, "lav_attention_bwd_bias: null pointer");
    if (int rc = attn_prepare(d, "lav_attention_bwd_bias", a, problems, p)) return rc;
    LAV_REQUIRE(p.bias_split, "lav_attention_bwd_bias: window mode on the persistent (N <= 256, tables given) or large-window (N <= 768) path only");
    a.qkv = (const bf16_t*)qkv; a.dout = (const bf16_t*)dout; a.lse = (float*)lse; a.dbias = dbias_table;
    return attn_run(stream, a, problems, p, AP_BIAS, "lav_attention_bwd_bias");
}

// 1 when the bias-table gradient of this descriptor can run as its own launch (lav_attention_bwd with dbias_table = NULL, then
// lav_attention_bwd_bias on any stream that waits for it), 0 when lav_attention_bwd has to produce it.
extern "C" int lav_attention_bias_split(const lav_attn_desc* d) {
    AttnArgs a; int problems = 0;
    if (attn_setup(d, a, problems)) return 0;
    return attn_plan(a, problems, attn_sw).bias_split ? 1 : 0;
}

// probe hook: the launches the entry of `pass` would make for this descriptor, without making them (no device needed)
extern "C" int lav_attention_plan(const lav_attn_desc* d, int pass, lav_attn_launch_info* out, int max_out) {
    static const char* const kernels[AK_COUNT] = {"win_fwd3", "win_bwd1", "win_dbias3", "winl_fwd", "winl_dq", "winl_dkv", "winl_dbias", "seq_fwd3", "seq_dq3",
                                                  "seq_dkv3", "seql_fwd", "seql_dq", "seql_dkv", "attn_fwd_kernel", "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel"};
    static const char* const routes[AR_COUNT] = {"window persistent", "window large", "sequence one-image", "sequence chunked", "generic window", "generic sequence"};
    static const char* const entries[AP_COUNT] = {"lav_attention_fwd", "lav_attention_bwd", "lav_attention_bwd", "lav_attention_bwd_bias"};
    LAV_REQUIRE(pass >= 0 && pass < AP_COUNT, "lav_attention_plan: pass %d (0 forward, 1 backward, 2 backward with the bias-table gradient, 3 that gradient alone)", pass);
    LAV_REQUIRE(out || max_out <= 0, "lav_attention_plan: null output array");
    AttnArgs a; int problems = 0; AttnPlan p;
    if (int rc = attn_prepare(d, entries[pass], a, problems, p)) return rc;
    LAV_REQUIRE(pass != AP_BIAS || p.bias_split, "lav_attention_bwd_bias: window mode on the persistent (N <= 256, tables given) or large-window (N <= 768) path only");
    for (int i = 0; i < p.n[pass] && i < max_out; ++i) {
        const AttnLaunch& l = p.launch[pass][i];
        out[i] = {kernels[l.kern], routes[p.route], l.grid_x, l.grid_y, l.block, (unsigned)l.lds, l.split, p.delta_negated ? 1 : 0};
    }
    return p.n[pass];
}
