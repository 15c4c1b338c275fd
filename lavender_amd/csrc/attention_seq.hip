// Fusion-encoder (BERT) self-attention for gfx950, sequences of up to 288 tokens (the pre-training / retrieval / QA shapes:
// L = 250 video + 26..32 text tokens), head_dim 64, key mask, counter-hash dropout on P, optional seq2seq mask.
// Round-3 kernels, same rules as attention_win.hip:
//   * K and V (forward, dQ pass) or Q and dO (dK / dV pass) of a (sequence, head) problem arrive by global_load_lds into ONE
//     slot-swizzled LDS image each (128-byte rows = full cache lines of the token-major qkv tensor) that serves both the
//     ds_read_b128 fragment reads and the transposing ds_read_b64_tr_b16 reads; the image is waited for once per problem.
//     Nothing is staged through registers, no global load is consumed while a DMA is in flight.
//   * the additive key mask enters the score tile as the C operand of its first MFMA (forward / dQ) or as a per-wave constant
//     (dK / dV); delta enters dP the same way; the softmax row sum is one more MFMA against a one-row ones fragment.
//     VALU per score element: fma + exp (+ the dropout hash) + 1/2 max3 + cvt_pk.
//   * 256-thread workgroups, two per CU (74-76 KB of LDS each): while one waits for its next problem's image the other computes.
//     A workgroup walks problems blockIdx.x, blockIdx.x + gridDim.x, ...; its four waves take the 32-row tiles round-robin.
//   * the S tile of step t+1 is issued before the softmax of step t (matrix pipe under the VALU chain of the same wave).
// Longer sequences (the 757-token Swin-L-384 shape, up to 768) run the chunked kernels at the end of this file; beyond that the generic
// kernels of attention.hip.
#include "attn_common.h"

#define LOG2E 1.4426950408889634f
#define HD 64

__device__ __forceinline__ void sdma16(unsigned lds_dst, const void* sbase, unsigned voff) {
    unsigned keep_m0;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep_m0) : "v"(voff), "s"(lds_dst), "s"(sbase) : "memory");
}
__device__ __forceinline__ void sdma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

union SFrag { uint4 u; bf16x8 b; };
#define SZERO16 {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}

__device__ __forceinline__ float smax3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// transposing A-operand read (32 d-values d0 .. d0 + 31 x 16 rows) from a K-type (slot-swizzled) 128-byte-row image
__device__ __forceinline__ bf16x8 tr_frag_k64(const char* tile, int row_base, int d0, int lane) {
    const int i = lane & 15, dhalf = (lane >> 4) & 1, hi = lane >> 5;
    const int r = i >> 2, c = i & 3;
    const int dcol = d0 + 16 * dhalf + 4 * c;
    const int slot = dcol >> 3, sub = (dcol & 7) * 2;
    const int row0 = row_base + 4 * hi + r;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(tile + krow_off<64>(row0, slot) + sub));
    s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(tile + krow_off<64>(row0 + 8, slot) + sub));
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = lo; u.s.b = hi4;
    return u.v;
}

// DMA of one operand image: rows [0, nrow8 * 8) of a (sequence, head) slice, 1-KB pieces of 8 rows x 128 B; wave w moves pieces
// w, w + 4, ...  Rows past the sequence end re-read its last row (never used: masked keys / padded queries).
__device__ __forceinline__ void seq_dma_image(unsigned lds_img, const bf16_t* base, long ld, int L, int npiece, int wave, int lane) {
    for (int t = wave; t < npiece; t += 4) {
        const int row = min(t * 8 + (lane >> 3), L - 1);
        const int prow = t * 8 + (lane >> 3);
        const int lslot = (lane & 7) ^ swz64(prow);
        sdma16(lds_img + t * 1024, base, (unsigned)((row * ld + lslot * 8) * 2));
    }
}

// counter-hash dropout factor pair for two adjacent keys from one 32-bit word of the group hash (lav_hash64: one 64-bit hash per FOUR keys)
__device__ __forceinline__ void drop_word(uint32_t h, uint32_t thresh16, float inv, float& m0, float& m1) {
    m0 = (h & 0xffffu) >= thresh16 ? inv : 0.f;
    m1 = (h >> 16) >= thresh16 ? inv : 0.f;
}

// dK / dV pass: a lane holds ONE key and four queries per register group, and the dropout hash is per (query, group of FOUR keys) -- the four
// lanes of a quad (keys 4 g .. 4 g + 3) need the same four hashes, each lane the 16-bit field of its own key.  Lane c of the quad hashes query c
// (ONE hash per lane instead of four) and the quad transposes the 4 x 4 matrix of 16-bit fields in two exchange steps (lane ^ 1: v_perm_b32 on
// the halves, lane ^ 2: the words), 4 DPP moves + 4 selects: f[e] = field (key & 3) of hash(query e), the same bits the forward computes.
__device__ __forceinline__ uint32_t quad_xor1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /* quad_perm [1, 0, 3, 2] */, 0xf, 0xf, false); }
__device__ __forceinline__ uint32_t quad_xor2(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E /* quad_perm [2, 3, 0, 1] */, 0xf, 0xf, false); }
__device__ __forceinline__ void drop_fields4(uint32_t seed, uint32_t base, uint32_t nq, int c, uint32_t (&f)[4]) {
    // element e of the register group has hash index base + e * nq; c = key & 3 = lane & 3
    const uint2 h = lav_hash64(seed, base + (uint32_t)c * nq);
    // step 1 (partner lane ^ 1): even lanes keep the low halves of both, odd lanes the high halves -> (field c & 1 of rows 2 (c >> 1), 2 (c >> 1) + 1) in x,
    // (field 2 + (c & 1) of the same rows) in y
    const uint32_t sel = (c & 1) ? 0x03020706u : 0x05040100u;
    const uint32_t x1 = __builtin_amdgcn_perm(quad_xor1(h.x), h.x, sel), y1 = __builtin_amdgcn_perm(quad_xor1(h.y), h.y, sel);
    // step 2 (partner lane ^ 2): lanes 0, 1 take the x words (fields 0 / 1), lanes 2, 3 the y words (fields 2 / 3); rows 0, 1 from lanes 0 / 1, rows 2, 3 from lanes 2 / 3
    const uint32_t px = quad_xor2(x1), py = quad_xor2(y1);
    const uint32_t r01 = (c & 2) ? py : x1, r23 = (c & 2) ? y1 : px;
    f[0] = r01 & 0xffffu; f[1] = r01 >> 16; f[2] = r23 & 0xffffu; f[3] = r23 >> 16;
}

// ------------------------------------------------------------------------------------------------------
// forward.  LDS: K image | V image | additive key mask (fp32, 0 / -inf; -inf past the sequence end).
// ------------------------------------------------------------------------------------------------------
template <bool CAUSAL, bool DROP>
__global__ __launch_bounds__(256, 2) void seq_fwd3(AttnArgs a, int nprob) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;
    char* Vs = smem + SEQ3_IMG;
    float* kadd = (float*)(smem + 2 * SEQ3_IMG);
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, C = a.C, ld = 3 * C;
    const int nt = a.nqt, npiece = nt * 4;
    const float sc = a.d.scale * LOG2E;
    const float inv_keep = DROP ? 1.f / (1.f - a.d.dropout_p) : 1.f;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    bf16x8 ones0;
    {
        float e8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) e8[e] = j == 0 ? 1.f : 0.f;
        ones0 = pack_frag(e8);
    }
    for (int p = blockIdx.x; p < nprob; p += gridDim.x) {
        const int prob = p / a.d.heads, head = p - prob * a.d.heads;
        const bf16_t* qbase = a.qkv + (long)prob * N * ld + head * HD;
        __syncthreads();                                     // every wave is done with the previous problem's images
        seq_dma_image(lds0, qbase + C, ld, N, npiece, wave, lane);
        seq_dma_image(lds0 + SEQ3_IMG, qbase + 2 * C, ld, N, npiece, wave, lane);
        for (int k = tid; k < nt * 32; k += 256)
            kadd[k] = (k >= N || (a.d.key_mask && a.d.key_mask[(long)prob * N + k] == 0)) ? -INFINITY : 0.f;
        sdma_wait_all();
        __syncthreads();

        // One query tile: key tiles t0, t0 + tstep, ...  split = false: all of them, normalise and store.  split = true (the LAST query tile when
        // nt = 4 k + 1, e.g. the 9 tiles of a 282-token sequence): this wave took every fourth key tile; the four partial (m, l, O) states are
        // merged through LDS (the K / V images are dead by then).  Without the split the wave that owns tile 8 runs 27 (query, key) tile pairs
        // against 18 of the other three -- the workgroup waits for it; with it the loads are 21 / 20 / 20 / 20.
        auto run_q = [&](const int qt, const int t0, const int tstep, const bool split) {
            const int q = qt * 32 + j;
            const bool q_ok = q < N;
            const long qrow = (long)min(q, N - 1);
            bf16x8 qf[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) { SFrag f; f.u = *(const uint4*)(qbase + qrow * ld + ks * 16 + 8 * hi); qf[ks] = f.b; }
            f32x16 o0 = SZERO16, o1 = SZERO16, lacc = SZERO16;
            float m_run = -INFINITY;
            const uint32_t drow = ((uint32_t)(prob * a.d.heads + head) * (uint32_t)N + (uint32_t)q) * (uint32_t)a.NH;
            f32x16 sa, sb;
            auto qk = [&](int t, f32x16& s) {
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {             // C operand = additive mask of the tile's keys (rows of S^T)
                    const float4 m4 = *(const float4*)(kadd + t * 32 + 8 * r4 + 4 * hi);
                    s[4 * r4] = m4.x; s[4 * r4 + 1] = m4.y; s[4 * r4 + 2] = m4.z; s[4 * r4 + 3] = m4.w;
                }
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    bf16x8 kf = *(const bf16x8*)(Ks + krow_off<HD>(t * 32 + j, ks * 2 + hi));
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
                }
            };
            auto soft = [&](int t, f32x16& s) {
                if (CAUSAL) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kk = t * 32 + tile_row(r, hi);
                        if (kk >= a.d.causal_from && (q < a.d.causal_from || kk > q)) s[r] = -INFINITY;
                    }
                }
                float mx = smax3(s[0], s[1], s[2]);
#pragma unroll
                for (int r = 3; r < 15; r += 2) mx = smax3(mx, s[r], s[r + 1]);
                mx = fmaxf(mx, s[15]);
                mx = xhalf_max(mx) * sc;
                if (__any(mx > m_run)) {
                    const float m_new = fmaxf(m_run, mx);
                    const float alpha = fast_exp2(m_run - m_new);   // m_run = -inf -> 0; a fully masked prefix keeps m = -inf
                    lacc[0] *= alpha;
#pragma unroll
                    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
                    m_run = m_new;
                }
                const float nm = m_run == -INFINITY ? 0.f : -m_run;
                uint32_t pk[8], pd[8];
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const uint2 hq = DROP ? lav_hash64(a.d.seed, drow + (uint32_t)(t * 8 + 2 * r4 + hi)) : make_uint2(0u, 0u);   // keys t * 32 + 8 r4 + 4 hi .. + 3
#pragma unroll
                    for (int e2 = 0; e2 < 2; ++e2) {
                        const int r = r4 * 4 + 2 * e2;
                        const float p0 = fast_exp2(fmaf(s[r], sc, nm)), p1 = fast_exp2(fmaf(s[r + 1], sc, nm));
                        pk[r >> 1] = pack2(p0, p1);
                        if (DROP) {
                            float m0, m1;
                            drop_word(e2 ? hq.y : hq.x, a.thresh16, inv_keep, m0, m1);
                            pd[r >> 1] = pack2(p0 * m0, p1 * m1);
                        }
                    }
                }
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    SFrag pf, pq;
                    pf.u = make_uint4(pk[4 * sl], pk[4 * sl + 1], pk[4 * sl + 2], pk[4 * sl + 3]);
                    if (DROP) pq.u = make_uint4(pd[4 * sl], pd[4 * sl + 1], pd[4 * sl + 2], pd[4 * sl + 3]); else pq.u = pf.u;
                    lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones0, pf.b, lacc, 0, 0, 0);      // normaliser: the un-dropped P
                    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Vs, t * 32 + 16 * sl, 0, lane), pq.b, o0, 0, 0, 0);
                    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Vs, t * 32 + 16 * sl, 32, lane), pq.b, o1, 0, 0, 0);
                }
            };
            if (t0 < nt) qk(t0, sa);
#pragma unroll 1
            for (int t = t0; t < nt; t += 2 * tstep) {
                if (t + tstep < nt) qk(t + tstep, sb);
                soft(t, sa);
                if (t + tstep < nt) {
                    if (t + 2 * tstep < nt) qk(t + 2 * tstep, sa);
                    soft(t + tstep, sb);
                }
            }
            float l_tot = lower_half(lacc[0]);
            if (split) {
                __syncthreads();                             // every wave is done with the K / V images: their space takes the partial states
                float* part = (float*)smem + wave * 2048;    // [8][64 lanes][4] accumulator quads of this wave
                float* ml = (float*)smem + 4 * 2048;         // [4 waves][2][32]
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    *(float4*)(part + (r4 * 64 + lane) * 4) = make_float4(o0[4 * r4], o0[4 * r4 + 1], o0[4 * r4 + 2], o0[4 * r4 + 3]);
                    *(float4*)(part + ((4 + r4) * 64 + lane) * 4) = make_float4(o1[4 * r4], o1[4 * r4 + 1], o1[4 * r4 + 2], o1[4 * r4 + 3]);
                }
                if (hi == 0) { ml[wave * 64 + j] = m_run; ml[wave * 64 + 32 + j] = l_tot; }
                __syncthreads();
                float m_all = -INFINITY;
#pragma unroll
                for (int w = 0; w < 4; ++w) m_all = fmaxf(m_all, ml[w * 64 + j]);
                float sw[4];
                l_tot = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const float mw = ml[w * 64 + j];
                    sw[w] = mw == -INFINITY ? 0.f : fast_exp2(mw - m_all);
                    l_tot = fmaf(sw[w], ml[w * 64 + 32 + j], l_tot);
                }
                m_run = m_all;
                // this wave finishes accumulator quad `wave` of both halves: rows d = 8 wave + 4 hi .. + 3 (and + 32)
                float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const float4 u = *(const float4*)((const float*)smem + w * 2048 + (wave * 64 + lane) * 4);
                    const float4 v = *(const float4*)((const float*)smem + w * 2048 + ((4 + wave) * 64 + lane) * 4);
                    a0[0] = fmaf(sw[w], u.x, a0[0]); a0[1] = fmaf(sw[w], u.y, a0[1]); a0[2] = fmaf(sw[w], u.z, a0[2]); a0[3] = fmaf(sw[w], u.w, a0[3]);
                    a1[0] = fmaf(sw[w], v.x, a1[0]); a1[1] = fmaf(sw[w], v.y, a1[1]); a1[2] = fmaf(sw[w], v.z, a1[2]); a1[3] = fmaf(sw[w], v.w, a1[3]);
                }
                const float inv_ls = l_tot > 0.f ? 1.f / l_tot : 0.f;
                if (q_ok) {
                    bf16_t* op = a.o_w + ((long)prob * N + q) * C + head * HD;
                    uint2 w2;
                    w2.x = pack2(a0[0] * inv_ls, a0[1] * inv_ls); w2.y = pack2(a0[2] * inv_ls, a0[3] * inv_ls);
                    *(uint2*)(op + 8 * wave + 4 * hi) = w2;
                    w2.x = pack2(a1[0] * inv_ls, a1[1] * inv_ls); w2.y = pack2(a1[2] * inv_ls, a1[3] * inv_ls);
                    *(uint2*)(op + 32 + 8 * wave + 4 * hi) = w2;
                    if (a.lse && hi == 0 && wave == 0) a.lse[(long)p * a.Npad + q] = m_run + log2f(l_tot);
                }
                return;
            }
            const float inv_l = l_tot > 0.f ? 1.f / l_tot : 0.f;
            if (q_ok) {
                bf16_t* op = a.o_w + ((long)prob * N + q) * C + head * HD;
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    uint2 w;
                    w.x = pack2(o0[r4 * 4 + 0] * inv_l, o0[r4 * 4 + 1] * inv_l);
                    w.y = pack2(o0[r4 * 4 + 2] * inv_l, o0[r4 * 4 + 3] * inv_l);
                    *(uint2*)(op + 8 * r4 + 4 * hi) = w;
                    w.x = pack2(o1[r4 * 4 + 0] * inv_l, o1[r4 * 4 + 1] * inv_l);
                    w.y = pack2(o1[r4 * 4 + 2] * inv_l, o1[r4 * 4 + 3] * inv_l);
                    *(uint2*)(op + 32 + 8 * r4 + 4 * hi) = w;
                }
                if (a.lse && hi == 0) a.lse[(long)p * a.Npad + q] = m_run + log2f(l_tot);   // log2 domain
            }
        };
        const bool split_last = (nt & 3) == 1 && nt >= 5;
        const int nwhole = split_last ? nt - 1 : nt;
        for (int qt = wave; qt < nwhole; qt += 4) run_q(qt, 0, 1, false);
        if (split_last) run_q(nt - 1, wave, 4, true);
    }
}

// ------------------------------------------------------------------------------------------------------
// backward pass 1: dQ and delta[q] = sum_d dO[q,d] O[q,d] (stored as +delta behind the lse, as the generic kernels do).
// LDS: K image | V image | additive key mask.
// ------------------------------------------------------------------------------------------------------
template <bool CAUSAL, bool DROP>
__global__ __launch_bounds__(256, 2) void seq_dq3(AttnArgs a, int nprob, float* delta_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;
    char* Vs = smem + SEQ3_IMG;
    float* kadd = (float*)(smem + 2 * SEQ3_IMG);
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, C = a.C, ld = 3 * C;
    const int nt = a.nqt, npiece = nt * 4;
    const float sc = a.d.scale * LOG2E;
    const float inv_keep = DROP ? 1.f / (1.f - a.d.dropout_p) : 1.f;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    for (int p = blockIdx.x; p < nprob; p += gridDim.x) {
        const int prob = p / a.d.heads, head = p - prob * a.d.heads;
        const bf16_t* qbase = a.qkv + (long)prob * N * ld + head * HD;
        __syncthreads();
        seq_dma_image(lds0, qbase + C, ld, N, npiece, wave, lane);
        seq_dma_image(lds0 + SEQ3_IMG, qbase + 2 * C, ld, N, npiece, wave, lane);
        for (int k = tid; k < nt * 32; k += 256)
            kadd[k] = (k >= N || (a.d.key_mask && a.d.key_mask[(long)prob * N + k] == 0)) ? -INFINITY : 0.f;
        sdma_wait_all();
        __syncthreads();

        for (int qt = wave; qt < nt; qt += 4) {
            const int q = qt * 32 + j;
            const bool q_ok = q < N;
            const long qrow = (long)prob * N + min(q, N - 1);
            bf16x8 qf[4], dof[4];
            float dl = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                SFrag fq, fg, fo;
                fq.u = *(const uint4*)(a.qkv + qrow * ld + head * HD + ks * 16 + 8 * hi);
                fg.u = *(const uint4*)(a.dout + qrow * C + head * HD + ks * 16 + 8 * hi);
                fo.u = *(const uint4*)(a.out + qrow * C + head * HD + ks * 16 + 8 * hi);
                qf[ks] = fq.b; dof[ks] = fg.b;
                float gf[8], of[8];
                unpack8(fg.u, gf); unpack8(fo.u, of);
#pragma unroll
                for (int e = 0; e < 8; ++e) dl = fmaf(gf[e], of[e], dl);
            }
            dl = xhalf_add(dl);
            const float nl = q_ok ? -a.lse[(long)p * a.Npad + q] : -INFINITY;   // padded query: P = 0
            if (q_ok && hi == 0) delta_out[(long)p * a.Npad + q] = dl;
            const float ndl = -dl;
            const uint32_t drow = ((uint32_t)(prob * a.d.heads + head) * (uint32_t)N + (uint32_t)q) * (uint32_t)a.NH;
            f32x16 dq0 = SZERO16, dq1 = SZERO16;
            f32x16 sa, pa;
            auto front = [&](int t, f32x16& s, f32x16& dp) {
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const float4 m4 = *(const float4*)(kadd + t * 32 + 8 * r4 + 4 * hi);
                    s[4 * r4] = m4.x; s[4 * r4 + 1] = m4.y; s[4 * r4 + 2] = m4.z; s[4 * r4 + 3] = m4.w;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) dp[r] = DROP ? 0.f : ndl;     // without dropout delta rides in as the C operand
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int off = krow_off<HD>(t * 32 + j, ks * 2 + hi);
                    bf16x8 kf = *(const bf16x8*)(Ks + off);
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
                    bf16x8 vf = *(const bf16x8*)(Vs + off);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dof[ks], dp, 0, 0, 0);
                }
            };
            auto back = [&](int t, const f32x16& s, const f32x16& dp) {
                uint32_t dk[8];
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const uint2 hq = DROP ? lav_hash64(a.d.seed, drow + (uint32_t)(t * 8 + 2 * r4 + hi)) : make_uint2(0u, 0u);   // keys t * 32 + 8 r4 + 4 hi .. + 3
#pragma unroll
                    for (int e2 = 0; e2 < 2; ++e2) {
                        const int r = r4 * 4 + 2 * e2;
                        float p0 = fast_exp2(fmaf(s[r], sc, nl)), p1 = fast_exp2(fmaf(s[r + 1], sc, nl));
                        if (CAUSAL) {
                            const int kk = t * 32 + 8 * r4 + 4 * hi + 2 * e2;
                            if (kk >= a.d.causal_from && (q < a.d.causal_from || kk > q)) p0 = 0.f;
                            if (kk + 1 >= a.d.causal_from && (q < a.d.causal_from || kk + 1 > q)) p1 = 0.f;
                        }
                        if (DROP) {
                            float m0, m1;
                            drop_word(e2 ? hq.y : hq.x, a.thresh16, inv_keep, m0, m1);
                            dk[r >> 1] = pack2(p0 * fmaf(dp[r], m0, ndl), p1 * fmaf(dp[r + 1], m1, ndl));
                        } else {
                            dk[r >> 1] = pack2(p0 * dp[r], p1 * dp[r + 1]);
                        }
                    }
                }
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    SFrag df; df.u = make_uint4(dk[4 * sl], dk[4 * sl + 1], dk[4 * sl + 2], dk[4 * sl + 3]);
                    dq0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Ks, t * 32 + 16 * sl, 0, lane), df.b, dq0, 0, 0, 0);
                    dq1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Ks, t * 32 + 16 * sl, 32, lane), df.b, dq1, 0, 0, 0);
                }
            };
            // not software-pipelined (the second S / dP pair costs 32 registers and spills): the other workgroup of the CU covers
#pragma unroll 1
            for (int t = 0; t < nt; ++t) {
                front(t, sa, pa);
                back(t, sa, pa);
            }
            if (q_ok) {
                bf16_t* op = a.dqkv + qrow * ld + head * HD;
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    uint2 w;
                    w.x = pack2(dq0[r4 * 4 + 0] * a.d.scale, dq0[r4 * 4 + 1] * a.d.scale);
                    w.y = pack2(dq0[r4 * 4 + 2] * a.d.scale, dq0[r4 * 4 + 3] * a.d.scale);
                    *(uint2*)(op + 8 * r4 + 4 * hi) = w;
                    w.x = pack2(dq1[r4 * 4 + 0] * a.d.scale, dq1[r4 * 4 + 1] * a.d.scale);
                    w.y = pack2(dq1[r4 * 4 + 2] * a.d.scale, dq1[r4 * 4 + 3] * a.d.scale);
                    *(uint2*)(op + 32 + 8 * r4 + 4 * hi) = w;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// backward pass 2: dK, dV.  Wave owns 32-key tiles, loops over the queries.  LDS: Q image | dO image | lse (+inf for padded
// queries) | delta.
// ------------------------------------------------------------------------------------------------------
template <bool CAUSAL, bool DROP>
__global__ __launch_bounds__(256, 2) void seq_dkv3(AttnArgs a, int nprob, const float* delta_in) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qs = smem;
    char* Gs = smem + SEQ3_IMG;
    float* qlse = (float*)(smem + 2 * SEQ3_IMG);
    float* qdl = qlse + SEQ3_ROWS;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, C = a.C, ld = 3 * C;
    const int nt = a.nqt, npiece = nt * 4;
    const float sc = a.d.scale * LOG2E;
    const float inv_keep = DROP ? 1.f / (1.f - a.d.dropout_p) : 1.f;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    for (int p = blockIdx.x; p < nprob; p += gridDim.x) {
        const int prob = p / a.d.heads, head = p - prob * a.d.heads;
        const bf16_t* qbase = a.qkv + (long)prob * N * ld + head * HD;
        __syncthreads();
        seq_dma_image(lds0, qbase, ld, N, npiece, wave, lane);
        seq_dma_image(lds0 + SEQ3_IMG, a.dout + (long)prob * N * C + head * HD, C, N, npiece, wave, lane);
        for (int k = tid; k < nt * 32; k += 256) {
            qlse[k] = k < N ? a.lse[(long)p * a.Npad + k] : INFINITY;     // padded query rows: P = exp2(v - inf) = 0
            qdl[k] = k < N ? delta_in[(long)p * a.Npad + k] : 0.f;
        }
        sdma_wait_all();
        __syncthreads();

        for (int kt = wave; kt < nt; kt += 4) {
            const int key = kt * 32 + j;
            const bool k_ok = key < N;
            const long krow = (long)prob * N + min(key, N - 1);
            const float k_add = (!k_ok || (a.d.key_mask && a.d.key_mask[(long)prob * N + min(key, N - 1)] == 0)) ? -INFINITY : 0.f;
            bf16x8 kf[4], vf[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                SFrag fk, fv;
                fk.u = *(const uint4*)(a.qkv + krow * ld + C + head * HD + ks * 16 + 8 * hi);
                fv.u = *(const uint4*)(a.qkv + krow * ld + 2 * C + head * HD + ks * 16 + 8 * hi);
                kf[ks] = fk.b; vf[ks] = fv.b;
            }
            f32x16 kadd16;
#pragma unroll
            for (int r = 0; r < 16; ++r) kadd16[r] = k_add;
            f32x16 dk0 = SZERO16, dk1 = SZERO16, dv0 = SZERO16, dv1 = SZERO16;
            const uint32_t dcol = (uint32_t)(prob * a.d.heads + head) * (uint32_t)N;
            const uint32_t sh = (uint32_t)(key & 1) * 16u;
#pragma unroll 1
            for (int qt = 0; qt < nt; ++qt) {
                const int q0 = qt * 32;
                f32x16 s = kadd16, dp = SZERO16;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int off = krow_off<HD>(q0 + j, ks * 2 + hi);
                    bf16x8 qa = *(const bf16x8*)(Qs + off);
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], s, 0, 0, 0);
                    bf16x8 ga = *(const bf16x8*)(Gs + off);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga, vf[ks], dp, 0, 0, 0);
                }
                uint32_t pk[8], dsk[8];
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int qb = q0 + 8 * r4 + 4 * hi;
                    const float4 l4 = *(const float4*)(qlse + qb);
                    const float4 d4 = *(const float4*)(qdl + qb);
                    const float ls[4] = {l4.x, l4.y, l4.z, l4.w};
                    const float dls[4] = {d4.x, d4.y, d4.z, d4.w};
                    float pv[4], dsv[4];
                    uint32_t h4[4] = {0u, 0u, 0u, 0u};
                    if (DROP) drop_fields4(a.d.seed, (dcol + (uint32_t)qb) * (uint32_t)a.NH + (uint32_t)(key >> 2), (uint32_t)a.NH, lane & 3, h4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = r4 * 4 + e;
                        float pe = fast_exp2(fmaf(s[r], sc, -ls[e]));
                        if (CAUSAL) {
                            const int qq = qb + e;
                            if (key >= a.d.causal_from && (qq < a.d.causal_from || key > qq)) pe = 0.f;
                        }
                        float m = 1.f;
                        if (DROP) m = h4[e] >= a.thresh16 ? inv_keep : 0.f;
                        pv[e] = DROP ? pe * m : pe;
                        dsv[e] = pe * (DROP ? fmaf(dp[r], m, -dls[e]) : dp[r] - dls[e]);
                    }
                    pk[2 * r4] = pack2(pv[0], pv[1]); pk[2 * r4 + 1] = pack2(pv[2], pv[3]);
                    dsk[2 * r4] = pack2(dsv[0], dsv[1]); dsk[2 * r4 + 1] = pack2(dsv[2], dsv[3]);
                }
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    SFrag pf, df;
                    pf.u = make_uint4(pk[4 * sl], pk[4 * sl + 1], pk[4 * sl + 2], pk[4 * sl + 3]);
                    df.u = make_uint4(dsk[4 * sl], dsk[4 * sl + 1], dsk[4 * sl + 2], dsk[4 * sl + 3]);
                    dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Gs, q0 + 16 * sl, 0, lane), pf.b, dv0, 0, 0, 0);
                    dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Gs, q0 + 16 * sl, 32, lane), pf.b, dv1, 0, 0, 0);
                    dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Qs, q0 + 16 * sl, 0, lane), df.b, dk0, 0, 0, 0);
                    dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Qs, q0 + 16 * sl, 32, lane), df.b, dk1, 0, 0, 0);
                }
            }
            if (k_ok) {
                bf16_t* op = a.dqkv + krow * ld + head * HD;
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int d = 8 * r4 + 4 * hi;
                    uint2 w;
                    w.x = pack2(dk0[r4 * 4 + 0] * a.d.scale, dk0[r4 * 4 + 1] * a.d.scale);
                    w.y = pack2(dk0[r4 * 4 + 2] * a.d.scale, dk0[r4 * 4 + 3] * a.d.scale);
                    *(uint2*)(op + C + d) = w;
                    w.x = pack2(dk1[r4 * 4 + 0] * a.d.scale, dk1[r4 * 4 + 1] * a.d.scale);
                    w.y = pack2(dk1[r4 * 4 + 2] * a.d.scale, dk1[r4 * 4 + 3] * a.d.scale);
                    *(uint2*)(op + C + 32 + d) = w;
                    w.x = pack2(dv0[r4 * 4 + 0], dv0[r4 * 4 + 1]);
                    w.y = pack2(dv0[r4 * 4 + 2], dv0[r4 * 4 + 3]);
                    *(uint2*)(op + 2 * C + d) = w;
                    w.x = pack2(dv1[r4 * 4 + 0], dv1[r4 * 4 + 1]);
                    w.y = pack2(dv1[r4 * 4 + 2], dv1[r4 * 4 + 3]);
                    *(uint2*)(op + 2 * C + 32 + d) = w;
                }
            }
        }
    }
}

// ======================================================================================================
// Long sequences (288 < L <= 768: the 757-token Swin-L-384 fusion input): same tile code, but a (sequence, head) problem no
// longer fits LDS whole.  512-thread workgroups; a work item is (problem, part): wave w owns ONE 32-row tile, part * 8 + w
// (queries in the forward / dQ pass, keys in the dK / dV pass), so the per-tile state (output accumulators, running max) lives
// in registers across the whole walk, and the other operand streams through LDS in 256-row chunks, double-buffered: chunk
// c + 1 is in flight (global_load_lds) under chunk c's MFMAs.  LDS: [2][image A 32 KB | image B 32 KB] + per-row floats.
// ======================================================================================================
// DMA of rows [row0, row0 + 256) of an operand (clamped to the last row of the sequence): 32 one-KB pieces, 4 per wave
__device__ __forceinline__ void seql_dma_chunk(unsigned lds_img, const bf16_t* base, long ld, int L, int row0, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = wave * 4 + i;
        const int prow = t * 8 + (lane >> 3);
        const int row = min(row0 + prow, L - 1);
        const int lslot = (lane & 7) ^ swz64(prow);
        sdma16(lds_img + t * 1024, base, (unsigned)((row * ld + lslot * 8) * 2));
    }
}

template <bool CAUSAL, bool DROP>
__global__ __launch_bounds__(512) void seql_fwd(AttnArgs a, int nprob, int parts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* kadd = (float*)(smem + 2 * SEQL_BUF);
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, C = a.C, ld = 3 * C;
    const int nt = a.nqt, nch = (nt + 7) / 8;
    const float sc = a.d.scale * LOG2E;
    const float inv_keep = DROP ? 1.f / (1.f - a.d.dropout_p) : 1.f;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    bf16x8 ones0;
    {
        float e8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) e8[e] = j == 0 ? 1.f : 0.f;
        ones0 = pack_frag(e8);
    }
    for (int it = blockIdx.x; it < nprob * parts; it += gridDim.x) {
        const int p = it / parts, part = it - p * parts;
        const int prob = p / a.d.heads, head = p - prob * a.d.heads;
        const bf16_t* qbase = a.qkv + (long)prob * N * ld + head * HD;
        const int qt = part * 8 + wave;
        const bool active = qt < nt;                         // wave-uniform; idle waves still move their DMA pieces
        const int q = qt * 32 + j;
        const bool q_ok = active && q < N;
        const long qrow = (long)min(q, N - 1);
        bf16x8 qf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { SFrag f; f.u = *(const uint4*)(qbase + qrow * ld + ks * 16 + 8 * hi); qf[ks] = f.b; }
        __syncthreads();                                     // every wave is done with the previous item's LDS
        for (int k = tid; k < nt * 32; k += 512)
            kadd[k] = (k >= N || (a.d.key_mask && a.d.key_mask[(long)prob * N + k] == 0)) ? -INFINITY : 0.f;
        seql_dma_chunk(lds0, qbase + C, ld, N, 0, wave, lane);
        seql_dma_chunk(lds0 + SEQL_IMG, qbase + 2 * C, ld, N, 0, wave, lane);
        sdma_wait_all();
        __syncthreads();
        f32x16 o0 = SZERO16, o1 = SZERO16, lacc = SZERO16;
        float m_run = -INFINITY;
        const uint32_t drow = ((uint32_t)(prob * a.d.heads + head) * (uint32_t)N + (uint32_t)q) * (uint32_t)a.NH;
        for (int c = 0; c < nch; ++c) {
            const char* Ks = smem + (c & 1) * SEQL_BUF;
            const char* Vs = Ks + SEQL_IMG;
            if (c + 1 < nch) {
                seql_dma_chunk(lds0 + ((c + 1) & 1) * SEQL_BUF, qbase + C, ld, N, (c + 1) * SEQL_CH, wave, lane);
                seql_dma_chunk(lds0 + ((c + 1) & 1) * SEQL_BUF + SEQL_IMG, qbase + 2 * C, ld, N, (c + 1) * SEQL_CH, wave, lane);
            }
            const int ntc = min(8, nt - c * 8);
            if (active) {
                f32x16 sa, sb;
                auto qk = [&](int tl, f32x16& s) {
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const float4 m4 = *(const float4*)(kadd + (c * 8 + tl) * 32 + 8 * r4 + 4 * hi);
                        s[4 * r4] = m4.x; s[4 * r4 + 1] = m4.y; s[4 * r4 + 2] = m4.z; s[4 * r4 + 3] = m4.w;
                    }
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        bf16x8 kf = *(const bf16x8*)(Ks + krow_off<HD>(tl * 32 + j, ks * 2 + hi));
                        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
                    }
                };
                auto soft = [&](int tl, f32x16& s) {
                    const int t = c * 8 + tl;
                    if (CAUSAL) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int kk = t * 32 + tile_row(r, hi);
                            if (kk >= a.d.causal_from && (q < a.d.causal_from || kk > q)) s[r] = -INFINITY;
                        }
                    }
                    float mx = smax3(s[0], s[1], s[2]);
#pragma unroll
                    for (int r = 3; r < 15; r += 2) mx = smax3(mx, s[r], s[r + 1]);
                    mx = fmaxf(mx, s[15]);
                    mx = xhalf_max(mx) * sc;
                    if (__any(mx > m_run)) {
                        const float m_new = fmaxf(m_run, mx);
                        const float alpha = fast_exp2(m_run - m_new);
                        lacc[0] *= alpha;
#pragma unroll
                        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
                        m_run = m_new;
                    }
                    const float nm = m_run == -INFINITY ? 0.f : -m_run;
                    uint32_t pk[8], pd[8];
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const uint2 hq = DROP ? lav_hash64(a.d.seed, drow + (uint32_t)(t * 8 + 2 * r4 + hi)) : make_uint2(0u, 0u);   // keys t * 32 + 8 r4 + 4 hi .. + 3
#pragma unroll
                        for (int e2 = 0; e2 < 2; ++e2) {
                            const int r = r4 * 4 + 2 * e2;
                            const float p0 = fast_exp2(fmaf(s[r], sc, nm)), p1 = fast_exp2(fmaf(s[r + 1], sc, nm));
                            pk[r >> 1] = pack2(p0, p1);
                            if (DROP) {
                                float m0, m1;
                                drop_word(e2 ? hq.y : hq.x, a.thresh16, inv_keep, m0, m1);
                                pd[r >> 1] = pack2(p0 * m0, p1 * m1);
                            }
                        }
                    }
#pragma unroll
                    for (int sl = 0; sl < 2; ++sl) {
                        SFrag pf, pq;
                        pf.u = make_uint4(pk[4 * sl], pk[4 * sl + 1], pk[4 * sl + 2], pk[4 * sl + 3]);
                        if (DROP) pq.u = make_uint4(pd[4 * sl], pd[4 * sl + 1], pd[4 * sl + 2], pd[4 * sl + 3]); else pq.u = pf.u;
                        lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones0, pf.b, lacc, 0, 0, 0);
                        o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Vs, tl * 32 + 16 * sl, 0, lane), pq.b, o0, 0, 0, 0);
                        o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Vs, tl * 32 + 16 * sl, 32, lane), pq.b, o1, 0, 0, 0);
                    }
                };
                qk(0, sa);
#pragma unroll 1
                for (int tl = 0; tl < ntc; tl += 2) {
                    if (tl + 1 < ntc) qk(tl + 1, sb);
                    soft(tl, sa);
                    if (tl + 1 < ntc) {
                        if (tl + 2 < ntc) qk(tl + 2, sa);
                        soft(tl + 1, sb);
                    }
                }
            }
            sdma_wait_all();
            __syncthreads();
        }
        const float l_tot = lower_half(lacc[0]);
        const float inv_l = l_tot > 0.f ? 1.f / l_tot : 0.f;
        if (q_ok) {
            bf16_t* op = a.o_w + ((long)prob * N + q) * C + head * HD;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                uint2 w;
                w.x = pack2(o0[r4 * 4 + 0] * inv_l, o0[r4 * 4 + 1] * inv_l);
                w.y = pack2(o0[r4 * 4 + 2] * inv_l, o0[r4 * 4 + 3] * inv_l);
                *(uint2*)(op + 8 * r4 + 4 * hi) = w;
                w.x = pack2(o1[r4 * 4 + 0] * inv_l, o1[r4 * 4 + 1] * inv_l);
                w.y = pack2(o1[r4 * 4 + 2] * inv_l, o1[r4 * 4 + 3] * inv_l);
                *(uint2*)(op + 32 + 8 * r4 + 4 * hi) = w;
            }
            if (a.lse && hi == 0) a.lse[(long)p * a.Npad + q] = m_run + log2f(l_tot);
        }
    }
}

template <bool CAUSAL, bool DROP>
__global__ __launch_bounds__(512) void seql_dq(AttnArgs a, int nprob, int parts, float* delta_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* kadd = (float*)(smem + 2 * SEQL_BUF);
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, C = a.C, ld = 3 * C;
    const int nt = a.nqt, nch = (nt + 7) / 8;
    const float sc = a.d.scale * LOG2E;
    const float inv_keep = DROP ? 1.f / (1.f - a.d.dropout_p) : 1.f;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    for (int it = blockIdx.x; it < nprob * parts; it += gridDim.x) {
        const int p = it / parts, part = it - p * parts;
        const int prob = p / a.d.heads, head = p - prob * a.d.heads;
        const bf16_t* qbase = a.qkv + (long)prob * N * ld + head * HD;
        const int qt = part * 8 + wave;
        const bool active = qt < nt;
        const int q = qt * 32 + j;
        const bool q_ok = active && q < N;
        const long qrow = (long)prob * N + min(q, N - 1);
        bf16x8 qf[4], dof[4];
        float dl = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            SFrag fq, fg, fo;
            fq.u = *(const uint4*)(a.qkv + qrow * ld + head * HD + ks * 16 + 8 * hi);
            fg.u = *(const uint4*)(a.dout + qrow * C + head * HD + ks * 16 + 8 * hi);
            fo.u = *(const uint4*)(a.out + qrow * C + head * HD + ks * 16 + 8 * hi);
            qf[ks] = fq.b; dof[ks] = fg.b;
            float gf[8], of[8];
            unpack8(fg.u, gf); unpack8(fo.u, of);
#pragma unroll
            for (int e = 0; e < 8; ++e) dl = fmaf(gf[e], of[e], dl);
        }
        dl = xhalf_add(dl);
        const float nl = q_ok ? -a.lse[(long)p * a.Npad + q] : -INFINITY;
        if (q_ok && hi == 0) delta_out[(long)p * a.Npad + q] = dl;
        const float ndl = -dl;
        __syncthreads();
        for (int k = tid; k < nt * 32; k += 512)
            kadd[k] = (k >= N || (a.d.key_mask && a.d.key_mask[(long)prob * N + k] == 0)) ? -INFINITY : 0.f;
        seql_dma_chunk(lds0, qbase + C, ld, N, 0, wave, lane);
        seql_dma_chunk(lds0 + SEQL_IMG, qbase + 2 * C, ld, N, 0, wave, lane);
        sdma_wait_all();
        __syncthreads();
        const uint32_t drow = ((uint32_t)(prob * a.d.heads + head) * (uint32_t)N + (uint32_t)q) * (uint32_t)a.NH;
        f32x16 dq0 = SZERO16, dq1 = SZERO16;
        for (int c = 0; c < nch; ++c) {
            const char* Ks = smem + (c & 1) * SEQL_BUF;
            const char* Vs = Ks + SEQL_IMG;
            if (c + 1 < nch) {
                seql_dma_chunk(lds0 + ((c + 1) & 1) * SEQL_BUF, qbase + C, ld, N, (c + 1) * SEQL_CH, wave, lane);
                seql_dma_chunk(lds0 + ((c + 1) & 1) * SEQL_BUF + SEQL_IMG, qbase + 2 * C, ld, N, (c + 1) * SEQL_CH, wave, lane);
            }
            const int ntc = min(8, nt - c * 8);
            if (active) {
#pragma unroll 1
                for (int tl = 0; tl < ntc; ++tl) {
                    const int t = c * 8 + tl;
                    f32x16 s, dp;
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const float4 m4 = *(const float4*)(kadd + t * 32 + 8 * r4 + 4 * hi);
                        s[4 * r4] = m4.x; s[4 * r4 + 1] = m4.y; s[4 * r4 + 2] = m4.z; s[4 * r4 + 3] = m4.w;
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) dp[r] = DROP ? 0.f : ndl;
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        const int off = krow_off<HD>(tl * 32 + j, ks * 2 + hi);
                        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(Ks + off), qf[ks], s, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(Vs + off), dof[ks], dp, 0, 0, 0);
                    }
                    uint32_t dk[8];
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const uint2 hq = DROP ? lav_hash64(a.d.seed, drow + (uint32_t)(t * 8 + 2 * r4 + hi)) : make_uint2(0u, 0u);   // keys t * 32 + 8 r4 + 4 hi .. + 3
#pragma unroll
                        for (int e2 = 0; e2 < 2; ++e2) {
                            const int r = r4 * 4 + 2 * e2;
                            float p0 = fast_exp2(fmaf(s[r], sc, nl)), p1 = fast_exp2(fmaf(s[r + 1], sc, nl));
                            if (CAUSAL) {
                                const int kk = t * 32 + 8 * r4 + 4 * hi + 2 * e2;
                                if (kk >= a.d.causal_from && (q < a.d.causal_from || kk > q)) p0 = 0.f;
                                if (kk + 1 >= a.d.causal_from && (q < a.d.causal_from || kk + 1 > q)) p1 = 0.f;
                            }
                            if (DROP) {
                                float m0, m1;
                                drop_word(e2 ? hq.y : hq.x, a.thresh16, inv_keep, m0, m1);
                                dk[r >> 1] = pack2(p0 * fmaf(dp[r], m0, ndl), p1 * fmaf(dp[r + 1], m1, ndl));
                            } else {
                                dk[r >> 1] = pack2(p0 * dp[r], p1 * dp[r + 1]);
                            }
                        }
                    }
#pragma unroll
                    for (int sl = 0; sl < 2; ++sl) {
                        SFrag df; df.u = make_uint4(dk[4 * sl], dk[4 * sl + 1], dk[4 * sl + 2], dk[4 * sl + 3]);
                        dq0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Ks, tl * 32 + 16 * sl, 0, lane), df.b, dq0, 0, 0, 0);
                        dq1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Ks, tl * 32 + 16 * sl, 32, lane), df.b, dq1, 0, 0, 0);
                    }
                }
            }
            sdma_wait_all();
            __syncthreads();
        }
        if (q_ok) {
            bf16_t* op = a.dqkv + qrow * ld + head * HD;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                uint2 w;
                w.x = pack2(dq0[r4 * 4 + 0] * a.d.scale, dq0[r4 * 4 + 1] * a.d.scale);
                w.y = pack2(dq0[r4 * 4 + 2] * a.d.scale, dq0[r4 * 4 + 3] * a.d.scale);
                *(uint2*)(op + 8 * r4 + 4 * hi) = w;
                w.x = pack2(dq1[r4 * 4 + 0] * a.d.scale, dq1[r4 * 4 + 1] * a.d.scale);
                w.y = pack2(dq1[r4 * 4 + 2] * a.d.scale, dq1[r4 * 4 + 3] * a.d.scale);
                *(uint2*)(op + 32 + 8 * r4 + 4 * hi) = w;
            }
        }
    }
}

// dK / dV: wave owns key tile part * 8 + w; Q and dO stream through LDS in 256-query chunks; lse (+inf for padded queries) and
// delta of the whole sequence sit behind the buffers.
template <bool CAUSAL, bool DROP>
__global__ __launch_bounds__(512) void seql_dkv(AttnArgs a, int nprob, int parts, const float* delta_in) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qlse = (float*)(smem + 2 * SEQL_BUF);
    float* qdl = qlse + SEQL_ROWS;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, C = a.C, ld = 3 * C;
    const int nt = a.nqt, nch = (nt + 7) / 8;
    const float sc = a.d.scale * LOG2E;
    const float inv_keep = DROP ? 1.f / (1.f - a.d.dropout_p) : 1.f;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    for (int it = blockIdx.x; it < nprob * parts; it += gridDim.x) {
        const int p = it / parts, part = it - p * parts;
        const int prob = p / a.d.heads, head = p - prob * a.d.heads;
        const bf16_t* qbase = a.qkv + (long)prob * N * ld + head * HD;
        const bf16_t* gbase = a.dout + (long)prob * N * C + head * HD;
        const int kt = part * 8 + wave;
        const bool active = kt < nt;
        const int key = kt * 32 + j;
        const bool k_ok = active && key < N;
        const long krow = (long)prob * N + min(key, N - 1);
        const float k_add = (!k_ok || (a.d.key_mask && a.d.key_mask[(long)prob * N + min(key, N - 1)] == 0)) ? -INFINITY : 0.f;
        bf16x8 kf[4], vf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            SFrag fk, fv;
            fk.u = *(const uint4*)(a.qkv + krow * ld + C + head * HD + ks * 16 + 8 * hi);
            fv.u = *(const uint4*)(a.qkv + krow * ld + 2 * C + head * HD + ks * 16 + 8 * hi);
            kf[ks] = fk.b; vf[ks] = fv.b;
        }
        __syncthreads();
        for (int k = tid; k < nt * 32; k += 512) {
            qlse[k] = k < N ? a.lse[(long)p * a.Npad + k] : INFINITY;
            qdl[k] = k < N ? delta_in[(long)p * a.Npad + k] : 0.f;
        }
        seql_dma_chunk(lds0, qbase, ld, N, 0, wave, lane);
        seql_dma_chunk(lds0 + SEQL_IMG, gbase, C, N, 0, wave, lane);
        sdma_wait_all();
        __syncthreads();
        f32x16 kadd16;
#pragma unroll
        for (int r = 0; r < 16; ++r) kadd16[r] = k_add;
        f32x16 dk0 = SZERO16, dk1 = SZERO16, dv0 = SZERO16, dv1 = SZERO16;
        const uint32_t dcol = (uint32_t)(prob * a.d.heads + head) * (uint32_t)N;
        const uint32_t sh = (uint32_t)(key & 1) * 16u;
        for (int c = 0; c < nch; ++c) {
            const char* Qs = smem + (c & 1) * SEQL_BUF;
            const char* Gs = Qs + SEQL_IMG;
            if (c + 1 < nch) {
                seql_dma_chunk(lds0 + ((c + 1) & 1) * SEQL_BUF, qbase, ld, N, (c + 1) * SEQL_CH, wave, lane);
                seql_dma_chunk(lds0 + ((c + 1) & 1) * SEQL_BUF + SEQL_IMG, gbase, C, N, (c + 1) * SEQL_CH, wave, lane);
            }
            const int ntc = min(8, nt - c * 8);
            if (active) {
#pragma unroll 1
                for (int tl = 0; tl < ntc; ++tl) {
                    const int q0 = (c * 8 + tl) * 32, l0 = tl * 32;
                    f32x16 s = kadd16, dp = SZERO16;
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        const int off = krow_off<HD>(l0 + j, ks * 2 + hi);
                        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(Qs + off), kf[ks], s, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(Gs + off), vf[ks], dp, 0, 0, 0);
                    }
                    uint32_t pk[8], dsk[8];
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const int qb = q0 + 8 * r4 + 4 * hi;
                        const float4 l4 = *(const float4*)(qlse + qb);
                        const float4 d4 = *(const float4*)(qdl + qb);
                        const float ls[4] = {l4.x, l4.y, l4.z, l4.w};
                        const float dls[4] = {d4.x, d4.y, d4.z, d4.w};
                        float pv[4], dsv[4];
                        uint32_t h4[4] = {0u, 0u, 0u, 0u};
                        if (DROP) drop_fields4(a.d.seed, (dcol + (uint32_t)qb) * (uint32_t)a.NH + (uint32_t)(key >> 2), (uint32_t)a.NH, lane & 3, h4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int r = r4 * 4 + e;
                            float pe = fast_exp2(fmaf(s[r], sc, -ls[e]));
                            if (CAUSAL) {
                                const int qq = qb + e;
                                if (key >= a.d.causal_from && (qq < a.d.causal_from || key > qq)) pe = 0.f;
                            }
                            float m = 1.f;
                            if (DROP) m = h4[e] >= a.thresh16 ? inv_keep : 0.f;
                            pv[e] = DROP ? pe * m : pe;
                            dsv[e] = pe * (DROP ? fmaf(dp[r], m, -dls[e]) : dp[r] - dls[e]);
                        }
                        pk[2 * r4] = pack2(pv[0], pv[1]); pk[2 * r4 + 1] = pack2(pv[2], pv[3]);
                        dsk[2 * r4] = pack2(dsv[0], dsv[1]); dsk[2 * r4 + 1] = pack2(dsv[2], dsv[3]);
                    }
#pragma unroll
                    for (int sl = 0; sl < 2; ++sl) {
                        SFrag pf, df;
                        pf.u = make_uint4(pk[4 * sl], pk[4 * sl + 1], pk[4 * sl + 2], pk[4 * sl + 3]);
                        df.u = make_uint4(dsk[4 * sl], dsk[4 * sl + 1], dsk[4 * sl + 2], dsk[4 * sl + 3]);
                        dv0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Gs, l0 + 16 * sl, 0, lane), pf.b, dv0, 0, 0, 0);
                        dv1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Gs, l0 + 16 * sl, 32, lane), pf.b, dv1, 0, 0, 0);
                        dk0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Qs, l0 + 16 * sl, 0, lane), df.b, dk0, 0, 0, 0);
                        dk1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_k64(Qs, l0 + 16 * sl, 32, lane), df.b, dk1, 0, 0, 0);
                    }
                }
            }
            sdma_wait_all();
            __syncthreads();
        }
        if (k_ok) {
            bf16_t* op = a.dqkv + krow * ld + head * HD;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int d = 8 * r4 + 4 * hi;
                uint2 w;
                w.x = pack2(dk0[r4 * 4 + 0] * a.d.scale, dk0[r4 * 4 + 1] * a.d.scale);
                w.y = pack2(dk0[r4 * 4 + 2] * a.d.scale, dk0[r4 * 4 + 3] * a.d.scale);
                *(uint2*)(op + C + d) = w;
                w.x = pack2(dk1[r4 * 4 + 0] * a.d.scale, dk1[r4 * 4 + 1] * a.d.scale);
                w.y = pack2(dk1[r4 * 4 + 2] * a.d.scale, dk1[r4 * 4 + 3] * a.d.scale);
                *(uint2*)(op + C + 32 + d) = w;
                w.x = pack2(dv0[r4 * 4 + 0], dv0[r4 * 4 + 1]);
                w.y = pack2(dv0[r4 * 4 + 2], dv0[r4 * 4 + 3]);
                *(uint2*)(op + 2 * C + d) = w;
                w.x = pack2(dv1[r4 * 4 + 0], dv1[r4 * 4 + 1]);
                w.y = pack2(dv1[r4 * 4 + 2], dv1[r4 * 4 + 3]);
                *(uint2*)(op + 2 * C + 32 + d) = w;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// one planned launch (attn_plan: grid, block, LDS bytes, parts) of the kernel's <CAUSAL, DROP> instantiation
template <bool CAUSAL, bool DROP>
static void seq_launch_as(hipStream_t s, const AttnArgs& a, const AttnLaunch& l, float* delta) {
    const int nprob = a.d.n_seq * a.d.heads;
    switch (l.kern) {
    case AK_SEQ_FWD3: attn_launch(seq_fwd3<CAUSAL, DROP>, l, s, a, nprob); break;
    case AK_SEQ_DQ3: attn_launch(seq_dq3<CAUSAL, DROP>, l, s, a, nprob, delta); break;
    case AK_SEQ_DKV3: attn_launch(seq_dkv3<CAUSAL, DROP>, l, s, a, nprob, delta); break;
    case AK_SEQL_FWD: attn_launch(seql_fwd<CAUSAL, DROP>, l, s, a, nprob, l.split); break;
    case AK_SEQL_DQ: attn_launch(seql_dq<CAUSAL, DROP>, l, s, a, nprob, l.split, delta); break;
    default: attn_launch(seql_dkv<CAUSAL, DROP>, l, s, a, nprob, l.split, delta); break;
    }
}
void seq_launch(hipStream_t s, const AttnArgs& a, const AttnPlan&, const AttnLaunch& l, float* delta) {
    const bool causal = a.d.causal_from > 0, drop = a.d.dropout_p > 0.f;
    if (causal) { if (drop) seq_launch_as<true, true>(s, a, l, delta); else seq_launch_as<true, false>(s, a, l, delta); }
    else { if (drop) seq_launch_as<false, true>(s, a, l, delta); else seq_launch_as<false, false>(s, a, l, delta); }
}
