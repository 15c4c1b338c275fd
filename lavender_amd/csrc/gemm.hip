// bf16 MFMA GEMM for gfx950 with fused epilogues.  One kernel template covers the three operand
// layouts the LAVENDER step needs:
//   NT  C[M,N] = A[M,K] . B[N,K]^T      forward linears (x . W^T)
//   NN  C[M,N] = A[M,K] . B[K,N]        input gradients (dY . W)
//   TN  C[M,N] = A[K,M]^T . B[K,N]      weight gradients (dY^T . X), split over the contraction
// Tile 128x128x64, 256 threads = 4 waves (2x2), each wave 64x64 = 4x4 v_mfma_f32_16x16x32_bf16.
// K-contiguous operands sit in LDS as [row][64] with an XOR swizzle of the 16-B slot (conflict-free
// ds_read_b128); contraction-strided operands sit as [16-col subtile][k][16] and are read with
// ds_read_b64_tr_b16 (hardware transpose).  The accumulator tile is staged through LDS (fp32) so the
// epilogue (bias / GELU / dropout / drop-path scale / residual / column sums) runs on 8-wide row
// chunks with 16-byte global accesses.
#include "common.h"
#include <type_traits>
#include <stdlib.h>
#include <math.h>
#include "../../include/lavender_hip.h"

#define BM 128
#define BN 128
#define BKT 64
#define NT_ 256
#define CSTRIDE 132
#define GEMM_LDS_BYTES (BM * CSTRIDE * 4)

struct GemmArgs {
    const bf16_t* A; const bf16_t* B; void* C;
    long lda, ldb, ldc;
    int M, N, K;
    int k_per_split;
    lav_gemm_epilogue e;
    uint32_t drop_thresh;
    int splits;           // grid = tiles * splits blocks (1-D)
    float* ws;            // split-K partial tiles [split][tile][128][128] fp32 (out_mode 2, splits > 1), or NULL
    int ws_tiles;         // tiles per split in ws
    int owner;            // out_mode 2 with one block per output tile: plain read-modify-write instead of atomics
    int group_n;          // > 0: tiles are walked in column groups of this many tiles (B panels of a group stay in the XCD's L2)
    int dbg;              // probe only (lav_gemm_select(5, v), wrong results): 1 = return before the epilogue, 2 = skip the k-loop, 4 = skip the epilogue's staging writes
    int nb_rows;          // > 0: B has only this many valid rows while N was rounded up to a multiple of 8 (lav_gemm_epilogue.c_pad_writable):
                          // B row reads and bias reads are clamped to it, the extra output columns receive unspecified values
    int assign;           // out_mode 2 (weight gradients): C = result instead of C += result (owner tiles and the split-K reduction pass)
    int nt_preact;        // store the saved-for-backward GELU' tensor with non-temporal stores (it is not read again before the backward:
                          // keeping it out of L2 / MALL is worth 0.6 ms per cfg2 step; LAV_NT_STORES=0 turns it off)
};

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ s16x4 tr_read(const char* lds_base, int off) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds_base + off));
}

// LDS images of one operand tile (16 KB):
//   K-contiguous operand : [128 rows][64 k] bf16, 128-byte rows, 16-byte slot s stored at s ^ (row & 7)
//                          -> ds_read_b128 fragment reads are bank-conflict-free
//   contraction-strided  : [64 k][128 n] bf16, 256-byte rows, 32-byte chunk c stored at c ^ skey(k)
//                          -> the four k-rows x 32 B that one ds_read_b64_tr_b16 lane group gathers, and the two
//                             groups of a 32-lane half, land on 8 distinct chunks = all 64 banks
// Both images are "row-linear up to a permutation inside the row", so a tile can be filled either through
// registers (edge tiles: zero fill, drop-path row skipping) or by global_load_lds (1 KB per wave-instruction,
// LDS address = base + lane*16) with the inverse permutation applied to the per-lane SOURCE address.
__device__ __forceinline__ int skey(int k) { return (k & 3) | (((k >> 3) & 1) << 2); }

// ---- global -> registers (one 128x64 or 64x128 operand tile = 4 x 16 B per thread) -------------
// keep-mask of one k-tile (drop-path row skipping, TN only): a 64-row tile spans at most two samples
// (rows_per_group >= 64), so the mask is "rows below kb use keep0, the rest keep1" -- scalars, no per-load division.
struct KeepInfo { int kb; bool k0, k1; };

template <bool KCONTIG>
__device__ __forceinline__ void tile_load(uint4 (&r)[4], const bf16_t* __restrict__ P, long ld, int o0, int O,
                                          int k0, int kend, int tid, const KeepInfo& ki) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int c = tid + NT_ * j;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (KCONTIG) {
            int row = c >> 3, slot = c & 7;
            int go = o0 + row, gk = k0 + slot * 8;
            if (go < O && gk < kend) v = *(const uint4*)(P + (long)go * ld + gk);
        } else {
            int krow = c >> 4, n8 = c & 15;
            int gk = k0 + krow, go = o0 + n8 * 8;
            bool ok = gk < kend && go < O && (gk < ki.kb ? ki.k0 : ki.k1);
            if (ok) v = *(const uint4*)(P + (long)gk * ld + go);
        }
        r[j] = v;
    }
}

template <bool KCONTIG>
__device__ __forceinline__ void tile_store(const uint4 (&r)[4], char* lds, int tid) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int c = tid + NT_ * j;
        int off;
        if (KCONTIG) {
            int row = c >> 3, slot = c & 7;
            off = row * 128 + ((slot ^ (row & 7)) << 4);
        } else {
            int krow = c >> 4, n8 = c & 15;
            off = krow * 256 + (((n8 >> 1) ^ skey(krow)) << 5) + (n8 & 1) * 16;
        }
        *(uint4*)(lds + off) = r[j];
    }
}

// ---- global -> LDS without registers: 4 wave-instructions per wave per operand tile ----------------
// Only for full k-tiles; rows / columns past the operand's extent are clamped to a valid address (they only feed
// output rows / columns that the epilogue masks).
template <bool KCONTIG>
__device__ __forceinline__ void tile_glds(char* lds, const bf16_t* __restrict__ P, long ld, int o0, int O, int k0, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = wave * 4 + i;
        const bf16_t* src;
        if (KCONTIG) {
            int row = min(o0 + t * 8 + (lane >> 3), O - 1);
            int slot = (lane & 7) ^ ((lane >> 3) & 7);
            src = P + (long)row * ld + k0 + slot * 8;
        } else {
            int krow = t * 4 + (lane >> 4);
            int ch = ((lane & 15) >> 1) ^ skey(krow);
            int col = min(o0 + ch * 16 + (lane & 1) * 8, ((O + 7) & ~7) - 8);
            src = P + (long)(k0 + krow) * ld + col;
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(lds + t * 1024), 16, 0, 0);
    }
}

// ---- LDS -> MFMA fragment: 16 rows (or cols) x 32 k; lane (i = l&15, g = l>>4) gets k = 8g..8g+7 ----
template <bool KCONTIG>
__device__ __forceinline__ bf16x8 frag_read(const char* lds, int t16, int ks, int lane) {
    if (KCONTIG) {
        int row = t16 * 16 + (lane & 15);
        int slot = ks * 4 + (lane >> 4);
        return *(const bf16x8*)(lds + row * 128 + ((slot ^ (row & 7)) << 4));
    } else {
        int i = lane & 15, g = lane >> 4, r = i >> 2, c = i & 3;
        int k = ks * 32 + 8 * g + r;                       // rows k..k+3 via lanes r=0..3 of the group; second read k+4
        int ch = (t16 ^ skey(k)) << 5;                     // skey(k) == skey(k + 4)
        s16x4 lo = tr_read(lds, k * 256 + ch + c * 8);
        s16x4 hi = tr_read(lds, (k + 4) * 256 + ch + c * 8);
        union { struct { s16x4 a, b; } s; bf16x8 v; } u;
        u.s.a = lo; u.s.b = hi;
        return u.v;
    }
}

// ---- fused epilogue over the fp32 accumulator tile staged in LDS (row stride CSTRIDE): all NTHR threads, 8-wide
// row chunks, 16-byte global accesses.  Order: alpha, bias, [preact], GELU, GELU', dropout, drop-path scale,
// residual, [column sums], store.
// F = compile-time feature mask: the large-tile kernels are instantiated for the handful of epilogue shapes the
// training step uses, so that each runs straight-line code (the all-features version is ~600 basic blocks of
// uniform branches and costs more than the k-loop on the short-K GEMMs of this model).
enum : unsigned { EF_BIAS = 1, EF_ACT = 2, EF_GIN = 4, EF_DROP = 8, EF_RSCALE = 16, EF_RES = 32, EF_COLSUM = 64,
                  EF_O32 = 128,        // fp32 store (the fp32 residual stream of the fusion encoder); the residual's own type is a run-time flag
                  EF_TNFLUSH = 0x4000, EF_GENERIC = 0x8000, EF_ALL = 0xFFFF };

// CH = 16-byte chunks per staged row (16: a 128-column block-wide tile; 8: a 64-column tile private to ONE wave -- then
// NTHR == 64, `cl` is that wave's LDS slice with row stride CSTR and nothing here synchronises the block).
// Per-(wave, tile) epilogue state that does not depend on the row chunk: the lane's 8 columns of bias / LayerNorm affine, and the running
// column sums.  The wave-private epilogues walk a tile in 2-4 row chunks; loading these once per tile (epi_begin) instead of once per
// chunk takes a dependent global load (and, for the column sums, an LDS reduction + 64 atomics) out of every chunk.
struct EpiState { float bias[8], lng[8], lnb[8], csum[8]; };

template <int ROWS, int NTHR, unsigned F = EF_ALL, int CH = 16, int CSTR = CSTRIDE>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& g, float* cl, int m0, int n0, int split, EpiState& st, const int phase) {
    // phase (a compile-time constant at every call site): bit 0 = (re)load the per-tile state into `st` before the rows, bit 1 = flush
    // the column sums after the rows (first chunk: 1, middle chunks: 0, last chunk: 2, self-contained call: 3)
    constexpr bool WAVE = CH != 16;
    constexpr int RPP = NTHR / CH;                          // rows per pass
    const lav_gemm_epilogue& e = g.e;
    if constexpr (F == EF_TNFLUSH) {
        // weight-gradient flush only: alpha * acc -> split-K workspace tile | owned read-modify-write | fp32 atomics
        const int etid = threadIdx.x, cc = etid & 15, gcol = n0 + cc * 8;
        const int ncols = min(8, g.N - gcol);
        constexpr int NIT = ROWS / (NTHR / 16);
        float* wsp = g.ws ? g.ws + ((long)split * g.ws_tiles + (long)(m0 / ROWS) * ((g.N + BN - 1) / BN) + n0 / BN) * (ROWS * BN) + cc * 8
                          : nullptr;
#pragma unroll 4
        for (int j = 0; j < NIT; ++j) {
            const int row = (etid >> 4) + (NTHR / 16) * j, grow = m0 + row;
            if (grow >= g.M || ncols <= 0) continue;
            float4 a = *(const float4*)&cl[row * CSTRIDE + cc * 8], b = *(const float4*)&cl[row * CSTRIDE + cc * 8 + 4];
            a.x *= e.alpha; a.y *= e.alpha; a.z *= e.alpha; a.w *= e.alpha; b.x *= e.alpha; b.y *= e.alpha; b.z *= e.alpha; b.w *= e.alpha;
            if (wsp) {
                *(float4*)(wsp + row * BN) = a; *(float4*)(wsp + row * BN + 4) = b;
            } else {
                float* p = (float*)g.C + (long)grow * g.ldc + gcol;
                if (g.owner && ncols == 8) {
                    if (g.assign) { *(float4*)p = a; *(float4*)(p + 4) = b; }       // first writer of the step: no read, C need not be zero
                    else {
                        float4 c = *(float4*)p, d = *(float4*)(p + 4);
                        c.x += a.x; c.y += a.y; c.z += a.z; c.w += a.w; d.x += b.x; d.y += b.y; d.z += b.z; d.w += b.w;
                        *(float4*)p = c; *(float4*)(p + 4) = d;
                    }
                } else {
                    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                    if (g.owner) { for (int x = 0; x < ncols; ++x) p[x] = g.assign ? v[x] : p[x] + v[x]; }
                    else for (int x = 0; x < ncols; ++x) atomicAdd(p + x, v[x]);
                }
            }
        }
        return;
    }
    constexpr bool GEN = (F & EF_GENERIC) != 0;
    const bool has_bias = (F & EF_BIAS) && e.bias;
    const bool has_gelu = (F & EF_ACT) && e.act == 1;
    const bool has_gin = (F & EF_GIN) && e.gelu_in;
    const bool has_drop = (F & EF_DROP) && e.dropout_p > 0.f;
    const bool has_rscale = (F & EF_RSCALE) && e.row_scale;
    const bool has_res = (F & EF_RES) && e.residual;
    const bool has_colsum = (F & EF_COLSUM) && e.colsum;
    const int etid = WAVE ? (threadIdx.x & 63) : threadIdx.x;
    const int cc = etid % CH;
    const int gcol = n0 + cc * 8;
    float (&csum)[8] = st.csum;
    float (&bias)[8] = st.bias;
    float (&lng)[8] = st.lng;
    float (&lnb)[8] = st.lnb;
    const int ncols = min(8, g.N - gcol);              // <=0: chunk outside
    // bf16 output addressing: element (row, gcol + x) at C + row * out_rs + out_c0 + x.  Head-major (lav_gemm_epilogue.hm_*): the 8 columns of a
    // chunk lie inside one head (hm_head_dim % 8 == 0), whose block is [hm_rows][hm_head_dim]
    long out_rs = g.ldc, out_c0 = gcol;
    if (e.hm_heads > 0) {
        const int hw = e.hm_heads * e.hm_head_dim, pl = gcol / hw, hc = gcol - pl * hw;
        out_rs = e.hm_head_dim;
        out_c0 = ((long)(pl * e.hm_heads + hc / e.hm_head_dim) * e.hm_rows) * e.hm_head_dim + hc % e.hm_head_dim;
    }
    const bool has_resln = (GEN || (F & EF_O32)) && (F & EF_RES) && e.residual && e.residual_f32 && e.res_ln_mean;
    if (phase & 1) {
#pragma unroll
        for (int x = 0; x < 8; ++x) { csum[x] = 0.f; bias[x] = 0.f; lng[x] = 1.f; lnb[x] = 0.f; }
        if (has_bias && ncols > 0) {
#pragma unroll
            for (int x = 0; x < 8; ++x)
                if (x < ncols && (g.nb_rows == 0 || gcol + x < g.nb_rows)) bias[x] = e.bias[gcol + x];
        }
        // LayerNorm of the residual rows (res_ln_*): this thread's 8 columns of gamma / beta, once
        if (has_resln && ncols > 0) {
#pragma unroll
            for (int x = 0; x < 8; ++x)
                if (x < ncols) { lng[x] = e.res_ln_gamma[gcol + x]; lnb[x] = e.res_ln_beta[gcol + x]; }
        }
    }
    // specialised variants are only dispatched when N % 8 == 0: a chunk is whole or outside the matrix, so past the
    // "outside" test every access is a full 16-byte one (compile-time) -- the preloads below run BEFORE that test
    const bool full = GEN ? ncols == 8 : true;
    const bool inside = GEN ? ncols == 8 : ncols > 0;
    constexpr int NIT = ROWS / RPP;
    constexpr int GRP = NIT < 4 ? NIT : 4;                 // rows handled together: their gelu_in / residual loads are
    static_assert(NIT % GRP == 0, "epilogue row grouping");  // issued back-to-back so HBM latency is paid once per group
#pragma unroll 1
    for (int j0 = 0; j0 < NIT; j0 += GRP) {
        uint4 pre_g[GRP], pre_r[GRP], pre_r2[GRP];
#pragma unroll
        for (int u = 0; u < GRP; ++u) {
            const int grow = m0 + etid / CH + RPP * (j0 + u);
            pre_g[u] = make_uint4(0, 0, 0, 0); pre_r[u] = pre_g[u]; pre_r2[u] = pre_g[u];
            if (inside && grow < g.M) {
                if (has_gin) {
                    if (e.gelu_in_is_grad == 2) {                 // one byte per element (see gq_pack8)
                        const uint2 q = *(const uint2*)((const uint8_t*)e.gelu_in + (long)grow * e.ldg + gcol);
                        pre_g[u].x = q.x; pre_g[u].y = q.y;
                    } else {
                        const uint4* gp = (const uint4*)((const bf16_t*)e.gelu_in + (long)grow * e.ldg + gcol);
                        if (g.nt_preact & 2) {               // LAV_NT_STORES & 4: the saved GELU' is read here for the LAST time -- stream it past L2 / MALL
                            typedef uint32_t lav_u32x4 __attribute__((ext_vector_type(4)));
                            const lav_u32x4 q = __builtin_nontemporal_load((const lav_u32x4*)gp);
                            pre_g[u] = make_uint4(q.x, q.y, q.z, q.w);
                        } else pre_g[u] = *gp;
                    }
                }
                if (has_res) {
                    const long rrow = e.res_rowmap ? e.res_rowmap[grow] : grow;
                    if (e.residual_f32 == 2) {
                        pre_r[u] = *(const uint4*)((const _Float16*)e.residual + rrow * e.ldr + gcol);      // fp16 rows: one 16-byte chunk
                    } else if (e.residual_f32) {
                        const float* rp = (const float*)e.residual + rrow * e.ldr + gcol;
                        pre_r[u] = *(const uint4*)rp; pre_r2[u] = *(const uint4*)(rp + 4);
                    } else {
                        pre_r[u] = *(const uint4*)((const bf16_t*)e.residual + rrow * e.ldr + gcol);
                    }
                }
            }
        }
#pragma unroll
      for (int u = 0; u < GRP; ++u) {
        const int j = j0 + u;
        const int row = etid / CH + RPP * j;
        const int grow = m0 + row;
        if (grow >= g.M || ncols <= 0) continue;
        float v[8];
        *(float4*)&v[0] = *(const float4*)&cl[row * CSTR + cc * 8];
        *(float4*)&v[4] = *(const float4*)&cl[row * CSTR + cc * 8 + 4];
#pragma unroll
        for (int x = 0; x < 8; ++x) v[x] = v[x] * e.alpha + bias[x];
        if (GEN && e.preact && !e.preact_is_grad) {
            bf16_t* p = (bf16_t*)e.preact + (long)grow * e.ldp + gcol;
            if (full) *(uint4*)p = pack8(v);
            else for (int x = 0; x < ncols; ++x) p[x] = f2bf(v[x]);
        }
        if (has_gelu) {
            if (e.preact && e.preact_is_grad) {
                // GELU and GELU' share erf and exp: y = z Phi(z), y' = Phi(z) + z phi(z); y' is what the backward needs
                float gp[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) gelu_and_grad(v[x], v[x], gp[x]);
                if (e.preact_is_grad == 2) {
                    uint8_t* p = (uint8_t*)e.preact + (long)grow * e.ldp + gcol;
                    const uint2 q = gq_pack8(gp);
                    if (full) *(uint2*)p = q;
                    else for (int x = 0; x < ncols; ++x) p[x] = (uint8_t)(((x < 4 ? q.x : q.y) >> (8 * (x & 3))) & 0xffu);
                } else {
                    bf16_t* p = (bf16_t*)e.preact + (long)grow * e.ldp + gcol;
                    if (full) {
                        if (g.nt_preact & 1) {
                            typedef uint32_t lav_u32x4 __attribute__((ext_vector_type(4)));
                            const uint4 q = pack8(gp);
                            const lav_u32x4 qv = {q.x, q.y, q.z, q.w};
                            __builtin_nontemporal_store(qv, (lav_u32x4*)p);
                        } else *(uint4*)p = pack8(gp);
                    }
                    else for (int x = 0; x < ncols; ++x) p[x] = f2bf(gp[x]);
                }
            } else {
#pragma unroll
                for (int x = 0; x < 8; ++x) v[x] = gelu_f(v[x]);
            }
        }
        if (GEN && e.act == 2) {                                  // ReLU (score head, main_pretrain_task_specific.py:131)
            if (e.preact && e.preact_is_grad) {
                float gp[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) gp[x] = v[x] > 0.f ? 1.f : 0.f;
                bf16_t* p = (bf16_t*)e.preact + (long)grow * e.ldp + gcol;
                if (full) *(uint4*)p = pack8(gp);
                else for (int x = 0; x < ncols; ++x) p[x] = f2bf(gp[x]);
            }
#pragma unroll
            for (int x = 0; x < 8; ++x) v[x] = fmaxf(v[x], 0.f);
        }
        if (has_gin) {
            const bf16_t* p = (const bf16_t*)e.gelu_in + (long)grow * e.ldg + gcol;
            float h[8];
            if (e.gelu_in_is_grad == 2) {
                if (full) gq_unpack8(make_uint2(pre_g[u].x, pre_g[u].y), h);
                else for (int x = 0; x < 8; ++x)
                    h[x] = x < ncols ? fmaf((float)((const uint8_t*)e.gelu_in)[(long)grow * e.ldg + gcol + x], 1.0f / LAV_GQ_SCALE, -LAV_GQ_OFF) : 0.f;
            } else if (full) unpack8(pre_g[u], h);
            else for (int x = 0; x < 8; ++x) h[x] = x < ncols ? bf2f(p[x]) : 0.f;
            if (!GEN || e.gelu_in_is_grad) {
#pragma unroll
                for (int x = 0; x < 8; ++x) v[x] *= h[x];
            } else {
#pragma unroll
                for (int x = 0; x < 8; ++x) v[x] *= gelu_grad_f(h[x]);
            }
        }
        if (has_drop) {
            const float inv = 1.0f / (1.0f - e.dropout_p);
#pragma unroll
            for (int x = 0; x < 8; ++x)
                v[x] = lav_keep(e.seed, (uint32_t)grow * (uint32_t)g.N + (uint32_t)(gcol + x), g.drop_thresh) ? v[x] * inv : 0.f;
        }
        if (has_rscale) {
            const float s = e.row_scale[grow / e.rows_per_group];
#pragma unroll
            for (int x = 0; x < 8; ++x) v[x] *= s;
        }
        if (has_res) {
            const long rrow = (!full && e.res_rowmap) ? e.res_rowmap[grow] : grow;     // the full-chunk path used the preloaded rows
            const bf16_t* p = (const bf16_t*)e.residual + rrow * e.ldr + gcol;
            float h[8];
            if (e.residual_f32) {
                if (e.residual_f32 == 2) {
                    if (full) unpack8_h(pre_r[u], h);
                    else for (int x = 0; x < 8; ++x) h[x] = x < ncols ? (float)((const _Float16*)e.residual)[rrow * e.ldr + gcol + x] : 0.f;
                }
                else if (full) { *(uint4*)&h[0] = pre_r[u]; *(uint4*)&h[4] = pre_r2[u]; }
                else for (int x = 0; x < 8; ++x) h[x] = x < ncols ? ((const float*)e.residual)[rrow * e.ldr + gcol + x] : 0.f;
                if (has_resln) {                          // the residual is a pre-LayerNorm row: add LayerNorm(row) (ln_fwd_kernel's arithmetic)
                    const long lrow = e.res_rowmap ? e.res_rowmap[grow] : grow;
                    const float mu = e.res_ln_mean[lrow], rs = e.res_ln_rstd[lrow];
#pragma unroll
                    for (int x = 0; x < 8; ++x) h[x] = (h[x] - mu) * rs * lng[x] + lnb[x];
                }
            } else if (full) unpack8(pre_r[u], h);
            else for (int x = 0; x < 8; ++x) h[x] = x < ncols ? bf2f(p[x]) : 0.f;
#pragma unroll
            for (int x = 0; x < 8; ++x) v[x] += h[x];
        }
        if (has_colsum) {
#pragma unroll
            for (int x = 0; x < 8; ++x) csum[x] += v[x];
        }
        if (GEN && g.ws) {
            // split-K partial: plain coalesced stores into this block's private workspace tile (a reduction pass sums the
            // splits) -- fp32 atomics cost ~20 ps each on MI355X, a third of the GEMM time when every split flushes with them
            float* p = g.ws + ((long)split * g.ws_tiles + (long)(m0 / ROWS) * ((g.N + BN - 1) / BN) + n0 / BN) * (ROWS * BN)
                       + row * BN + cc * 8;
            *(float4*)p = *(float4*)&v[0]; *(float4*)(p + 4) = *(float4*)&v[4];
        } else if (GEN ? e.out_mode == 0 : !(F & EF_O32)) {
            bf16_t* p = (bf16_t*)g.C + (long)grow * out_rs + out_c0;      // row-major (ldc, gcol) or head-major (hm_head_dim, block base)
            if (full) *(uint4*)p = pack8(v);
            else for (int x = 0; x < ncols; ++x) p[x] = f2bf(v[x]);
        } else if (e.out_mode == 3) {                      // fp16 store (the residual stream as halves)
            _Float16* p = (_Float16*)g.C + (long)grow * g.ldc + gcol;
            if (full) *(uint4*)p = pack8_h(v);
            else for (int x = 0; x < ncols; ++x) p[x] = (_Float16)__builtin_amdgcn_fmed3f(v[x], -65504.f, 65504.f);
        } else if (!GEN || e.out_mode == 1) {
            float* p = (float*)g.C + (long)grow * g.ldc + gcol;
            if (full) { *(float4*)p = *(float4*)&v[0]; *(float4*)(p + 4) = *(float4*)&v[4]; }
            else for (int x = 0; x < ncols; ++x) p[x] = v[x];
        } else if (g.owner) {
            float* p = (float*)g.C + (long)grow * g.ldc + gcol;
            if (full) {
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
                if (!g.assign) { a = *(float4*)p; b = *(float4*)(p + 4); }
                a.x += v[0]; a.y += v[1]; a.z += v[2]; a.w += v[3]; b.x += v[4]; b.y += v[5]; b.z += v[6]; b.w += v[7];
                *(float4*)p = a; *(float4*)(p + 4) = b;
            } else for (int x = 0; x < ncols; ++x) p[x] = g.assign ? v[x] : p[x] + v[x];
        } else {
            float* p = (float*)g.C + (long)grow * g.ldc + gcol;
            for (int x = 0; x < ncols; ++x) atomicAdd(p + x, v[x]);
        }
      }
    }
    if (has_colsum && (phase & 2)) {
        constexpr int W = CH * 8;                           // staged tile width in columns
        if (WAVE) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); else __syncthreads();
        float* red = cl;                                  // [RPP][W]
#pragma unroll
        for (int x = 0; x < 8; ++x) red[(etid / CH) * W + cc * 8 + x] = csum[x];
        if (WAVE) { __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier(); } else __syncthreads();
        if (etid < W && n0 + etid < g.N) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < RPP; ++r) s += red[r * W + etid];
            atomicAdd(e.colsum + n0 + etid, s);
        }
    }
}

template <int ROWS, int NTHR, unsigned F = EF_ALL, int CH = 16, int CSTR = CSTRIDE>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& g, float* cl, int m0, int n0, int split = 0) {
    EpiState st;
    gemm_epilogue<ROWS, NTHR, F, CH, CSTR>(g, cl, m0, n0, split, st, 3);
}

// KG = number of 4-wave groups per block.  KG == 2 (weight gradients): the two groups walk alternate k-tiles of
// the SAME output tile with private LDS stages and merge their accumulators through LDS -- twice the waves per
// CU without doubling the number of fp32-atomic output tiles (the epilogue atomics are what caps split-K).
template <bool AK, bool BK, int KG, unsigned F = EF_ALL>
__global__ __launch_bounds__(NT_ * KG) void gemm_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem_all[];
    const int grp = KG == 1 ? 0 : (threadIdx.x >> 8);
    char* smem = smem_all + grp * 65536;
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // XCD-aware bijective remap: each XCD (block b -> XCD b % 8) walks a contiguous run of tiles, n fastest
    const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BM - 1) / BM;
    const int nwg = tiles_m * tiles_n;
    // 1-D grid of nwg * splits blocks; hardware block b runs on XCD b % 8.  The bijective remap gives each XCD one
    // contiguous run of (split, tile) work items, split-major: blocks that share a k-range (and so the same rows of both
    // operands) sit on the same XCD and hit in its L2 -- with the split on blockIdx.z every XCD pulled every k-range
    // (measured: ~1.2 GB of L2 fills for a dW GEMM whose operands total 276 MB).
    int bid = blockIdx.x;
    {
        const int tot = nwg * g.splits;
        int q = tot >> 3, r = tot & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int split = bid / nwg;
    bid -= split * nwg;
    const int m0 = (bid / tiles_n) * BM, n0 = (bid % tiles_n) * BN;
    const int kbeg = split * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);
    const int nk = (kend - kbeg + BKT - 1) / BKT;


    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // TN only: bias gradient = sum over the contraction of A's columns, computed on the matrix cores against a
    // ones fragment by the wn==0 waves of the n0==0 blocks (every column of the product equals the row sum)
    const bool do_rowsum = !AK && g.e.rowsum_a != nullptr && n0 == 0 && wn == 0;
    f32x4 acc1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc1[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 ones;
    {
        union { uint4 u; bf16x8 b; } o; o.u = make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u); ones = o.b;
    }

    uint4 ra[4], rb[4];
    const float* keep = g.e.k_keep;
    const int nit = (nk + KG - 1) / KG;                    // iterations per group (tiles kt = it*KG + grp; overrun tiles read as zeros)
    // per k-tile mode: 0 = every row dropped (skip loads and MFMAs), 1 = full tile, no masking: HBM -> LDS directly,
    // 2 = through registers (K tail, or a tile that straddles a kept and a dropped sample)
    KeepInfo ki; ki.kb = 0x7fffffff; ki.k0 = ki.k1 = true;
    auto tile_mode = [&](int k0, KeepInfo& o) {
        o.kb = 0x7fffffff; o.k0 = o.k1 = true;
        if (k0 >= kend) return 0;
        if (keep) {
            const int s0 = k0 / g.e.k_rows_per_group;
            o.kb = (s0 + 1) * g.e.k_rows_per_group;
            o.k0 = keep[s0] != 0.f;
            o.k1 = o.kb < min(k0 + BKT, kend) ? keep[s0 + 1] != 0.f : o.k0;
            if (!o.k0 && !o.k1) return 0;
            if (!o.k0 || !o.k1) return 2;
        }
        return k0 + BKT <= kend ? 1 : 2;
    };
    int mode_cur = 0;
    if (nk > 0) {
        const int k0 = __builtin_amdgcn_readfirstlane(kbeg + grp * BKT);
        mode_cur = tile_mode(k0, ki);
        if (mode_cur == 1) {
            tile_glds<AK>(smem, g.A, g.lda, m0, g.M, k0, wave, lane);
            tile_glds<BK>(smem + 16384, g.B, g.ldb, n0, g.N, k0, wave, lane);
        } else if (mode_cur == 2) {
            tile_load<AK>(ra, g.A, g.lda, m0, g.M, k0, kend, tid, ki);
            tile_load<BK>(rb, g.B, g.ldb, n0, g.N, k0, kend, tid, ki);
            tile_store<AK>(ra, smem, tid);
            tile_store<BK>(rb, smem + 16384, tid);
        }
    }
    __syncthreads();
    for (int it = 0; it < nit; ++it) {
        const int cur = it & 1;
        char* la = smem + cur * 32768;
        char* lb = la + 16384;
        const int k0n = __builtin_amdgcn_readfirstlane(kbeg + ((it + 1) * KG + grp) * BKT);
        const int mode_next = it + 1 < nit ? tile_mode(k0n, ki) : 0;
        if (mode_next == 1) {
            tile_glds<AK>(smem + (cur ^ 1) * 32768, g.A, g.lda, m0, g.M, k0n, wave, lane);
            tile_glds<BK>(smem + (cur ^ 1) * 32768 + 16384, g.B, g.ldb, n0, g.N, k0n, wave, lane);
        } else if (mode_next == 2) {
            tile_load<AK>(ra, g.A, g.lda, m0, g.M, k0n, kend, tid, ki);
            tile_load<BK>(rb, g.B, g.ldb, n0, g.N, k0n, kend, tid, ki);
        }
        if (mode_cur != 0) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 fa[4], fb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[i] = frag_read<AK>(la, wm * 4 + i, ks, lane);
#pragma unroll
                for (int j = 0; j < 4; ++j) fb[j] = frag_read<BK>(lb, wn * 4 + j, ks, lane);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
                if (!AK && do_rowsum) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc1[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], ones, acc1[i], 0, 0, 0);
                }
            }
        }
        if (mode_next == 2) {
            tile_store<AK>(ra, smem + (cur ^ 1) * 32768, tid);
            tile_store<BK>(rb, smem + (cur ^ 1) * 32768 + 16384, tid);
        }
        mode_cur = mode_next;
        __syncthreads();
    }

    if (!AK && do_rowsum && (lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                if (row < g.M) atomicAdd(g.e.rowsum_a + row, acc1[i][r] * g.e.alpha);
            }
    }
    // ---- stage the accumulator tile through LDS (fp32, row stride 132 floats) ----------------------
    float* cl = (float*)smem_all;
    if (KG == 1 || grp == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int row = wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                    int col = wn * 64 + j * 16 + (lane & 15);
                    cl[row * CSTRIDE + col] = acc[i][j][r];
                }
    }
    __syncthreads();
    if (KG == 2) {
        if (grp == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        int row = wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                        int col = wn * 64 + j * 16 + (lane & 15);
                        cl[row * CSTRIDE + col] += acc[i][j][r];
                    }
        }
        __syncthreads();
    }

    gemm_epilogue<BM, NT_ * KG, F>(g, cl, m0, n0, split);
}

// ------------------------------------------------------------------------------------------------------
// Large-M variant for the forward / input-gradient layouts (A K-contiguous): 256x128x64 tile, 512 threads = 8 waves
// (4 x 2, 64x64 each), THREE LDS stages filled only by global_load_lds.  Loads for k-tile t+2 are issued before the
// MFMAs of tile t and the single barrier per tile waits with a COUNTED vmcnt (the newest tile stays in flight), so
// HBM / L2 latency is covered by two tiles of compute instead of sitting behind every barrier.
// Requires K % 64 == 0 (true for every Swin-B / BERT shape; the 128x128 kernel handles the rest).
// ------------------------------------------------------------------------------------------------------
#define BIG_BM 256
#define BIG_STAGE 49152
#define BIG_LDS (3 * BIG_STAGE)

template <bool KCONTIG, int INSTR_PER_WAVE>
__device__ __forceinline__ void big_glds(char* lds, const bf16_t* __restrict__ P, long ld, int o0, int O, int k0, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < INSTR_PER_WAVE; ++i) {
        const int t = wave * INSTR_PER_WAVE + i;
        const bf16_t* src;
        if (KCONTIG) {
            int row = min(o0 + t * 8 + (lane >> 3), O - 1);
            int slot = (lane & 7) ^ ((lane >> 3) & 7);
            src = P + (long)row * ld + k0 + slot * 8;
        } else {
            int krow = t * 4 + (lane >> 4);
            int ch = ((lane & 15) >> 1) ^ skey(krow);
            int col = min(o0 + ch * 16 + (lane & 1) * 8, ((O + 7) & ~7) - 8);
            src = P + (long)(k0 + krow) * ld + col;
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(lds + t * 1024), 16, 0, 0);
    }
}

template <int IPW = 4>
__device__ __forceinline__ void huge_glds_strided(char* lds, const bf16_t* __restrict__ P, long ld, int o0, int O, int k0, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < IPW; ++i) {                        // [64 k][256 n] bf16, 512-byte rows, 2 rows per wave-instruction
        const int t = wave * IPW + i;
        const int krow = t * 2 + (lane >> 5);
        const int ch = ((lane & 31) >> 1) ^ skey(krow);
        const int col = min(o0 + ch * 16 + (lane & 1) * 8, ((O + 7) & ~7) - 8);
        const bf16_t* src = P + (long)(k0 + krow) * ld + col;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(lds + t * 1024), 16, 0, 0);
    }
}

// drop-path row skipping for the large-tile weight-gradient kernels (A tile = [64 k][256 m], 512-byte k-rows):
// returns 0 when every contraction row of the k-tile belongs to a dropped sample (skip the MFMAs), 1 when all rows are
// kept, 2 when the tile straddles a kept and a dropped sample -- then the dropped k-rows are zeroed in LDS.
__device__ __forceinline__ int tn_keep_mode(const lav_gemm_epilogue& e, int k0, int& kb, bool& keep0, bool& keep1) {
    const int s0 = k0 / e.k_rows_per_group;
    kb = (s0 + 1) * e.k_rows_per_group - k0;                 // rows [0, kb) of the tile belong to sample s0
    keep0 = e.k_keep[s0] != 0.f;
    keep1 = kb < BKT ? e.k_keep[s0 + 1] != 0.f : keep0;
    return (keep0 && keep1) ? 1 : (!keep0 && !keep1) ? 0 : 2;
}

template <int NTHR = 512>
__device__ __forceinline__ void tn_zero_a_rows(char* lds_a, int kb, bool keep0, bool keep1, int tid) {
#pragma unroll
    for (int p = 0; p < 2048 / NTHR; ++p) {
        const int krow = p * (NTHR / 32) + (tid >> 5);
        const bool keep = krow < kb ? keep0 : keep1;
        if (!keep) *(uint4*)(lds_a + krow * 512 + (tid & 31) * 16) = make_uint4(0, 0, 0, 0);
    }
}

__device__ __forceinline__ bf16x8 huge_frag_strided(const char* lds, int t16, int ks, int lane) {
    const int i = lane & 15, g = lane >> 4, r = i >> 2, c = i & 3;
    const int k = ks * 32 + 8 * g + r;
    const int ch = (t16 ^ skey(k)) << 5;
    s16x4 lo = tr_read(lds, k * 512 + ch + c * 8);
    s16x4 hi = tr_read(lds, (k + 4) * 512 + ch + c * 8);
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = lo; u.s.b = hi;
    return u.v;
}

template <bool AKC, bool BKC, unsigned F = EF_ALL>
__global__ __launch_bounds__(512) void gemm_big_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BIG_BM - 1) / BIG_BM;
    const int nwg = tiles_m * tiles_n;
    // 1-D grid of nwg * splits blocks; hardware block b runs on XCD b % 8.  The bijective remap gives each XCD one
    // contiguous run of (split, tile) work items, split-major: blocks that share a k-range (and so the same rows of both
    // operands) sit on the same XCD and hit in its L2 -- with the split on blockIdx.z every XCD pulled every k-range
    // (measured: ~1.2 GB of L2 fills for a dW GEMM whose operands total 276 MB).
    int bid = blockIdx.x;
    {
        const int tot = nwg * g.splits;
        int q = tot >> 3, r = tot & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int split = bid / nwg;
    bid -= split * nwg;
    const int m0 = (bid / tiles_n) * BIG_BM, n0 = (bid % tiles_n) * BN;
    const int kbeg = split * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);
    const int nk = (kend - kbeg) / BKT;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // TN: bias gradient on the matrix cores (ones fragment), wn == 0 waves of the n0 == 0 blocks
    const bool do_rowsum = !AKC && g.e.rowsum_a != nullptr && n0 == 0 && wn == 0;
    f32x4 acc1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc1[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 ones;
    {
        union { uint4 u; bf16x8 b; } o; o.u = make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u); ones = o.b;
    }

    auto issue = [&](int kt) {
        char* st = smem + (kt % 3) * BIG_STAGE;
        const int k0 = kbeg + kt * BKT;
        if (AKC) big_glds<true, 4>(st, g.A, g.lda, m0, g.M, k0, wave, lane);          // 256 rows x 128 B = 32 instr
        else huge_glds_strided(st, g.A, g.lda, m0, g.M, k0, wave, lane);              // [64 k][256 m], 32 instr
        big_glds<BKC, 2>(st + 32768, g.B, g.ldb, n0, g.nb_rows ? g.nb_rows : g.N, k0, wave, lane);   // 16 KB = 16 instr
    };
    if (nk > 0) issue(0);
    if (nk > 1) {
        issue(1);
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();

    for (int kt = 0; kt < nk; ++kt) {
        const char* la = smem + (kt % 3) * BIG_STAGE;
        const char* lb = la + 32768;
        const bool more = kt + 2 < nk;
        if (more) issue(kt + 2);
        int kmode = 1;
        if (!AKC && g.e.k_keep) {
            int kb; bool keep0, keep1;
            kmode = tn_keep_mode(g.e, kbeg + kt * BKT, kb, keep0, keep1);
            if (kmode == 2) {
                tn_zero_a_rows(const_cast<char*>(la), kb, keep0, keep1, tid);
                __syncthreads();
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (kmode == 0) break;
            bf16x8 fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[i] = AKC ? frag_read<true>(la, wm * 4 + i, ks, lane) : huge_frag_strided(la, wm * 4 + i, ks, lane);
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = frag_read<BKC>(lb, wn * 4 + j, ks, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
            if (!AKC && do_rowsum) {
#pragma unroll
                for (int i = 0; i < 4; ++i) acc1[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], ones, acc1[i], 0, 0, 0);
            }
        }
        // tile kt+1 must have landed (6 wave-instructions per tile per wave; keep tile kt+2 in flight)
        if (more) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    if (!AKC && do_rowsum && (lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                if (row < g.M) atomicAdd(g.e.rowsum_a + row, acc1[i][r] * g.e.alpha);
            }
    }

    if constexpr (F != EF_ALL && F != EF_TNFLUSH) {
        // specialised epilogues: each wave stages and stores its own 64 x 64 block through a private LDS slice (see the
        // 256x256 kernel) -- all operand stages were consumed before the loop's last barrier
        constexpr int WS = 68;
        float* clw = (float*)smem + wave * (64 * WS);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    clw[(i * 16 + (lane >> 4) * 4 + r) * WS + j * 16 + (lane & 15)] = acc[i][j][r];
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        gemm_epilogue<64, 64, F, 8, WS>(g, clw, m0 + wm * 64, n0 + wn * 64, split);
        return;
    }
    float* cl = (float*)smem;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row = wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                int col = wn * 64 + j * 16 + (lane & 15);
                cl[row * CSTRIDE + col] = acc[i][j][r];
            }
    __syncthreads();
    gemm_epilogue<BIG_BM, 512, F>(g, cl, m0, n0, split);
}

// ------------------------------------------------------------------------------------------------------
// 256x256x64 variant (N a multiple of 256, large M): 8 waves as 2 x 4, each 128x64 = 8x4 MFMA tiles (128
// accumulator registers).  PMC on the 256x128 kernel (8192^3): MFMA busy 41 %, waves 29 % in s_waitcnt/barrier --
// the per-CU L2->LDS stream (48 KB per 2*256*128*64 flop, 85 flop/B) is what paces it; the square tile moves 64 KB
// per 2x the flops (128 flop/B) and needs only two LDS stages because one tile of MFMAs (2176 cycles per SIMD)
// already covers the load latency.  The accumulator tile is handed to the epilogue in two 128-column halves.
// ------------------------------------------------------------------------------------------------------
#define HUGE_STAGE 65536
#define HUGE_LDS 139264   // max(2 stages of 64 KB, block-wide epilogue 256 x 132 floats, eight wave-private 64 x 68 float slices)

// NW = waves per block.  8: 2 x 4 waves of 128x64 (shipped).  Per k-tile the LDS pipe moves 192 KB of fragment reads +
// 64 KB of direct-to-LDS writes = 2048 clk, exactly the MFMA time -- the k-loop sits near 47 % of the MFMA peak.
// NW = 4 (2 x 2 waves of 128x128, 256 accumulator registers, one wave per SIMD, 128 KB of reads) was measured at HALF
// the rate: with a single wave per SIMD nothing covers the LDS latency between the compiler's read/MFMA groups.
// RF = 16-row fragments per wave: 8 -> 256-row tiles; 6 -> 192-row tiles (K-contiguous layouts with a specialised epilogue only):
// a 45120 x 768 output is 531 tiles of 256 x 256 = 2.07 rounds on 256 CUs (a third of the last round's CUs idle for a whole
// tile), but 705 tiles of 192 x 256 = 2.75 rounds of 3/4-size tiles.
template <bool AKC, bool BKC, unsigned F, int NW, int RF = 8, int BNT = 256, int LW = 0>
__device__ __forceinline__ void gemm_huge_body(const GemmArgs& g) {
    static_assert(LW == 0 || (AKC && BKC && NW == 8 && F != EF_ALL && F != EF_TNFLUSH), "loader waves: both operands K-contiguous, specialised epilogue");
    constexpr int BMT = 2 * RF * 16;                      // tile rows
    constexpr int IPA = BMT / 8 / NW;                     // direct-to-LDS wave-instructions per A tile per wave (K-contiguous A)
    static_assert(RF == 8 || (AKC && F != EF_ALL && F != EF_TNFLUSH), "192-row tiles: K-contiguous A, specialised epilogue");
    static_assert(BNT == 256 || (AKC && BKC && NW == 4 && F != EF_ALL && F != EF_TNFLUSH), "128-column tiles: 4 waves, both operands K-contiguous");
    constexpr int WN = NW / 2;                            // wave grid 2 (m) x WN (n)
    constexpr int NJ = BNT / 16 / WN;                     // 16-column fragments per wave
    constexpr int IPW = 32 / NW;                          // direct-to-LDS wave-instructions per operand tile per wave
    constexpr int IPB = BNT / 8 / NW;                     // ... per K-contiguous B tile per wave
    constexpr int BOFF = BNT == 256 ? 32768 : BMT * 128;  // B tile behind the A tile
    constexpr int STAGE = BNT == 256 ? HUGE_STAGE : (BMT + BNT) * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int tiles_n = g.N / BNT, tiles_m = (g.M + BMT - 1) / BMT;
    const int nwg = tiles_m * tiles_n;
    // 1-D grid of nwg * splits blocks; hardware block b runs on XCD b % 8.  The bijective remap gives each XCD one
    // contiguous run of (split, tile) work items, split-major: blocks that share a k-range (and so the same rows of both
    // operands) sit on the same XCD and hit in its L2 -- with the split on blockIdx.z every XCD pulled every k-range
    // (measured: ~1.2 GB of L2 fills for a dW GEMM whose operands total 276 MB).
    int bid = blockIdx.x;
    {
        const int tot = nwg * g.splits;
        int q = tot >> 3, r = tot & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int split = bid / nwg;
    bid -= split * nwg;
    int tm = bid / tiles_n, tn = bid % tiles_n;
    if (g.group_n > 0 && g.group_n < tiles_n) {
        const int per = tiles_m * g.group_n, cg = bid / per, rem = bid - cg * per;
        const int gw = min(g.group_n, tiles_n - cg * g.group_n);          // last group may be narrower
        tm = rem / gw; tn = cg * g.group_n + rem % gw;
    }
    const int m0 = tm * BMT, n0 = tn * BNT;
    const int kbeg = split * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);
    const int nk = (kend - kbeg) / BKT;

    if constexpr (LW > 0) {
        // Loader waves (wave >= NW): they issue EVERY direct-to-LDS instruction of the k-loop -- a global_load_lds issue holds its wave for
        // 60-185 cycles, time the eight compute waves then spend on fragment reads and MFMAs instead -- wait for their own loads and
        // meet the compute waves at the k-tile barrier; they leave before the (barrier-free) epilogue.
        if (wave >= NW) {
            const int lw = wave - NW;
            constexpr int PA = BMT / 8 / LW, PB = BNT / 8 / LW;
            const bf16_t* ar[PA];
            const bf16_t* br[PB];
            const int sw = ((lane & 7) ^ ((lane >> 3) & 7)) * 8;
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                int r = min(m0 + (lw * PA + i) * 8 + (lane >> 3), g.M - 1);
                if (g.e.a_rowmap) r = g.e.a_rowmap[r];
                ar[i] = g.A + (long)r * g.lda + sw;
            }
#pragma unroll
            for (int i = 0; i < PB; ++i) br[i] = g.B + (long)min(n0 + (lw * PB + i) * 8 + (lane >> 3), g.N - 1) * g.ldb + sw;
            auto load_tile = [&](int kt) {
                char* st = smem + (kt & 1) * STAGE;
                const int k0 = kbeg + kt * BKT;
#pragma unroll
                for (int i = 0; i < PA; ++i)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ar[i] + k0),
                                                     (__attribute__((address_space(3))) void*)(st + (lw * PA + i) * 1024), 16, 0, 0);
#pragma unroll
                for (int i = 0; i < PB; ++i)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(br[i] + k0),
                                                     (__attribute__((address_space(3))) void*)(st + BOFF + (lw * PB + i) * 1024), 16, 0, 0);
            };
            if (nk > 0) load_tile(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            for (int kt = 0; kt < nk; ++kt) {
                if (kt + 1 < nk) load_tile(kt + 1);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
            return;
        }
    }
    f32x4 acc[RF][NJ];
#pragma unroll
    for (int i = 0; i < RF; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // TN: bias gradient (row sums of A^T) on the matrix cores against a ones fragment, wn == 0 waves of the n0 == 0 blocks
    const bool do_rowsum = !AKC && g.e.rowsum_a != nullptr && n0 == 0 && wn == 0;
    f32x4 acc1[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc1[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 ones;
    {
        union { uint4 u; bf16x8 b; } o; o.u = make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u); ones = o.b;
    }

    // K-contiguous A through an optional row map (pair expansion, lav_gemm_epilogue.a_rowmap): a lane's IPA source rows are fixed
    // over the k-loop, so the map is read once here and the k-loop's DMA stream stays free of register-destination loads
    const bf16_t* arow[AKC ? IPA : 1];
    if constexpr (AKC) {
#pragma unroll
        for (int i = 0; i < IPA; ++i) {
            int r = min(m0 + (wave * IPA + i) * 8 + (lane >> 3), g.M - 1);
            if (g.e.a_rowmap) r = g.e.a_rowmap[r];
            arow[i] = g.A + (long)r * g.lda + ((lane & 7) ^ ((lane >> 3) & 7)) * 8;
        }
    }
    auto issue = [&](int kt) {
        char* st = smem + (kt & 1) * STAGE;
        const int k0 = kbeg + kt * BKT;
        if constexpr (AKC) {
#pragma unroll
            for (int i = 0; i < IPA; ++i)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(arow[i] + k0),
                                                 (__attribute__((address_space(3))) void*)(st + (wave * IPA + i) * 1024), 16, 0, 0);
        }
        else huge_glds_strided<IPW>(st, g.A, g.lda, m0, g.M, k0, wave, lane);
        if (BKC) big_glds<true, IPB>(st + BOFF, g.B, g.ldb, n0, g.N, k0, wave, lane);
        else huge_glds_strided<IPW>(st + BOFF, g.B, g.ldb, n0, g.N, k0, wave, lane);
    };
    if (LW == 0 && nk > 0) issue(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    for (int kt = 0; kt < ((g.dbg & 2) ? 0 : nk); ++kt) {
        const char* la = smem + (kt & 1) * STAGE;
        const char* lb = la + BOFF;
        if (LW == 0 && kt + 1 < nk) issue(kt + 1);
        int kmode = 1;
        if (!AKC && g.e.k_keep) {
            int kb; bool keep0, keep1;
            kmode = tn_keep_mode(g.e, kbeg + kt * BKT, kb, keep0, keep1);
            if (kmode == 2) {
                tn_zero_a_rows<NW * 64>(const_cast<char*>(la), kb, keep0, keep1, tid);
                __syncthreads();
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (kmode == 0) break;
            bf16x8 fa[RF], fb[NJ];
#pragma unroll
            for (int i = 0; i < RF; ++i) fa[i] = AKC ? frag_read<true>(la, wm * RF + i, ks, lane) : huge_frag_strided(la, wm * RF + i, ks, lane);
#pragma unroll
            for (int j = 0; j < NJ; ++j) fb[j] = BKC ? frag_read<true>(lb, wn * NJ + j, ks, lane) : huge_frag_strided(lb, wn * NJ + j, ks, lane);
#pragma unroll
            for (int i = 0; i < RF; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
            if constexpr (!AKC) if (do_rowsum) {
#pragma unroll
                for (int i = 0; i < 8; ++i) acc1[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], ones, acc1[i], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    if (!AKC && do_rowsum && (lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 128 + i * 16 + (lane >> 4) * 4 + r;
                if (row < g.M) atomicAdd(g.e.rowsum_a + row, acc1[i][r] * g.e.alpha);
            }
    }

    if (g.dbg & 1) return;
    if constexpr ((NW == 8 || BNT == 128) && F != EF_ALL && F != EF_TNFLUSH) {
        // specialised forward / input-gradient epilogues: every wave stages its own accumulator block through a private LDS slice
        // in 64- or 32-row chunks and stores it in full 128-byte row pieces -- no block barriers.  Round 3 tried the epilogue straight
        // from the accumulator registers (swapped MFMA operands + permuted B rows so that a lane holds row-contiguous columns, no LDS
        // round trip): with 32-byte pieces per row per store instruction the STEP was 5.5 ms slower (83.0 vs 77.5 ms; isolated
        // launches within +-3 %), with 64-byte pieces equal (77.9): partial-line writes and residual reads are what the step, run
        // next to the weight-gradient stream, cannot afford.  The LDS-staged full-line form stays.
        constexpr int WS = 68;                            // private row stride (floats)
        constexpr int CF = RF == 8 ? 4 : (RF % 2 == 0 ? 2 : 1); // 16-row fragments per staged chunk: 64-row halves (256-row tile), 32-row thirds, or single fragments
        float* clw = (float*)smem + wave * (64 * WS);
        EpiState es;                                       // bias / LayerNorm affine / column sums of this wave's 64 columns: once per tile
#pragma unroll
        for (int h = 0; h < RF / CF; ++h) {               // unrolled: acc[] must be indexed with compile-time constants
            if (!(g.dbg & 4)) {
#pragma unroll
            for (int i = 0; i < CF; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        clw[(i * 16 + (lane >> 4) * 4 + r) * WS + j * 16 + (lane & 15)] = acc[h * CF + i][j][r];
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);           // lgkmcnt(0): the slice is only read by this wave
            __builtin_amdgcn_wave_barrier();
            gemm_epilogue<CF * 16, 64, F, 8, WS>(g, clw, m0 + wm * (RF * 16) + h * (CF * 16), n0 + wn * 64, split, es,
                                                 (h == 0 ? 1 : 0) | (h == RF / CF - 1 ? 2 : 0));
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
        }
        return;
    }
    float* cl = (float*)smem;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        if (wn / (WN / 2) == h) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        int row = wm * 128 + i * 16 + (lane >> 4) * 4 + r;
                        int col = (wn % (WN / 2)) * (NJ * 16) + j * 16 + (lane & 15);
                        cl[row * CSTRIDE + col] = acc[i][j][r];
                    }
        }
        __syncthreads();
        gemm_epilogue<BIG_BM, NW * 64, F>(g, cl, m0, n0 + h * 128, split);
        __syncthreads();
    }
}

template <bool AKC, bool BKC, unsigned F = EF_ALL>
__global__ __launch_bounds__(512) void gemm_huge_kernel(GemmArgs g) { gemm_huge_body<AKC, BKC, F, 8>(g); }
template <bool AKC, bool BKC, unsigned F>
__global__ __launch_bounds__(512) void gemm_h192_kernel(GemmArgs g) { gemm_huge_body<AKC, BKC, F, 8, 6>(g); }
// 192 x 256 tiles, eight compute waves + two LOADER waves (640 threads; the 155 registers of the 192-row body fit three waves per SIMD).
// Bit-identical to gemm_h192_kernel; isolated -2 ... -12 % on the shapes the 192-row tile is chosen for (45120 x 768 x {768, 2304, 3072}: the
// longer K, the more), -0.2 ... -0.3 ms on the cfg2 step (at the edge of the run-to-run noise).  Forced on every 256-column shape (LAV_GEMM_H192L=2, tools/h192l_probe.py) it loses 5-50 %
// to the 256-row tile elsewhere.  The 256-row tile with loader waves (A fragments read four at a time to fit 168 registers: 164, no spills)
// won 2-9 % isolated on the wide fusion outputs and LOST 0.8 ms in the step (three resident waves per SIMD next to the weight-gradient
// stream), so it is not kept.
template <bool AKC, bool BKC, unsigned F>
__global__ __launch_bounds__(640) void gemm_h192l_kernel(GemmArgs g) { gemm_huge_body<AKC, BKC, F, 8, 6, 256, 2>(g); }
// ------------------------------------------------------------------------------------------------------
// Phase-shifted 256x256x64 kernel for the forward / input-gradient layout (round 6, gemm_ps_kernel).  Same tile, wave tiles, LDS images and
// epilogue as gemm_huge_kernel; what changes is WHEN a wave does what.  The two waves of a SIMD (w and w + 4: groups g = wave >> 2, rows
// [128 g, 128 g + 128) of the tile) run one barrier apart, as in the weight-gradient ping-pong kernel: while a group issues the 64 MFMAs of
// k-step t back to back from registers (all 24 fragments of a k-step are read beforehand: 96 registers), its SIMD partners read THEIR
// fragments of the next k-step from LDS and issue the operand DMA of the k-step after it -- in gemm_huge both waves of a SIMD issue their
// DMA pieces at the same moment (~1000 cycles per k-step during which the matrix pipe has no issuer) and wait for the same LDS round trips.
// Two 64 KB stages (k-tiles of 64: full 128-byte row pieces, unlike the k-tile-32 ring that tied in round 2): the group that reads a stage
// first (g = 0) brings its own A half and the shared B tile, two phases before it reads them; g = 1 brings its A half one phase later.
// Bit-identical to gemm_huge_kernel (same accumulation order).
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ps_dma(unsigned lds_dst, const void* sbase, unsigned voff) {
    unsigned keep_m0;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep_m0) : "v"(voff), "s"(lds_dst), "s"(sbase) : "memory");
}

// RF = 16-row fragments per wave: 8 -> 256-row tiles, 6 -> 192-row tiles (the shapes gemm_h192l_kernel serves: outputs that under-fill the last round of
// 256-row tiles); a group owns RF * 16 rows, its A half is 2 RF pieces of 8 rows.
template <unsigned F, int RF = 8>
__global__ __launch_bounds__(512) void gemm_ps_kernel(GemmArgs g) {
    static_assert(RF == 8 || RF == 6, "256- or 192-row tiles");
    constexpr int BMT = 2 * RF * 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wn = wave & 3;
    const int tiles_n = g.N / 256, tiles_m = (g.M + BMT - 1) / BMT;
    int bid = blockIdx.x;
    {
        const int tot = tiles_m * tiles_n;
        int q = tot >> 3, r = tot & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    int tm = bid / tiles_n, tn = bid % tiles_n;
    if (g.group_n > 0 && g.group_n < tiles_n) {
        const int per = tiles_m * g.group_n, cg = bid / per, rem = bid - cg * per;
        const int gw = min(g.group_n, tiles_n - cg * g.group_n);
        tm = rem / gw; tn = cg * g.group_n + rem % gw;
    }
    const int m0 = tm * BMT, n0 = tn * 256;
    const int nk = (g.dbg & 2) ? 0 : g.K / BKT;               // (probe bits as in gemm_huge_kernel: 2 = no k-loop, 1 = no epilogue -- timing only)

    // ---- operand DMA, eight pieces per wave and read phase.  Group 0 (reads a stage first) brings the shared B tile of the NEXT stage (its buffer is
    // free once group 1 has read the stage before: two phases to land).  Group 1 brings both A halves: its own of the next stage (two phases) and group
    // 0's of the stage after (that buffer half is free as soon as group 0 has read it: three phases).  Per-lane byte offsets relative to the operand
    // base (the caller keeps M * lda and N * ldb below 2^31 bytes).
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int swz = ((lane & 7) ^ ((lane >> 3) & 7)) * 16;
    constexpr int PH = RF * 2 / 4;                                       // pieces per wave of an A half: 4 (256-row tile) or 3 (192-row tile)
    unsigned voffA[2][PH];                                              // [half][piece]: group 1 uses both, group 0 only its own half (prologue)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < PH; ++i) {
            int r = min(m0 + (h * RF * 2 + wn * PH + i) * 8 + (lane >> 3), g.M - 1);
            if (g.e.a_rowmap) r = g.e.a_rowmap[r];
            voffA[h][i] = (unsigned)r * (unsigned)g.lda * 2u + (unsigned)swz;
        }
    const unsigned voffB = (unsigned)(n0 + wn * 64 + (lane >> 3)) * (unsigned)g.ldb * 2u + (unsigned)swz;
    auto issue_a = [&](int kt, int half) __attribute__((always_inline)) {
        const unsigned st = lds0 + (unsigned)(kt & 1) * HUGE_STAGE;
        const bf16_t* pa = g.A + (long)kt * BKT;
#pragma unroll
        for (int i = 0; i < PH; ++i) ps_dma(__builtin_amdgcn_readfirstlane(st + (half * RF * 2 + wn * PH + i) * 1024), pa, voffA[half][i]);
    };
    auto issue_b = [&](int kt) __attribute__((always_inline)) {
        const unsigned st = lds0 + (unsigned)(kt & 1) * HUGE_STAGE;
        const bf16_t* pb = g.B + (long)kt * BKT;
#pragma unroll
        for (int i = 0; i < 8; ++i) ps_dma(__builtin_amdgcn_readfirstlane(st + 32768 + (wn * 8 + i) * 1024), pb + (long)i * 8 * g.ldb, voffB);
    };

    f32x4 acc[RF][4];
#pragma unroll
    for (int i = 0; i < RF; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 fa[2][RF], fb[2][4];
    const int foff = (lane & 15) * 128, fsl = lane >> 4, fx = lane & 7;
    const int fo[2] = {foff + (((0 + fsl) ^ fx) << 4), foff + (((4 + fsl) ^ fx) << 4)};
    auto read = [&](int kt) __attribute__((always_inline)) {
        const char* st = smem + (kt & 1) * HUGE_STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int i = 0; i < RF; ++i) fa[ks][i] = *(const bf16x8*)(st + (grp * RF + i) * 2048 + fo[ks]);
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[ks][j] = *(const bf16x8*)(st + 32768 + (wn * 4 + j) * 2048 + fo[ks]);
        }
    };
    auto compute = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < RF; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[ks][i], fb[ks][j], acc[i][j], 0, 0, 0);
    };

    // phase fence: nothing moves across it -- without the sched_barriers hipcc pulls the MFMAs of the next compute phase up between the fragment
    // reads of the read phase (it recycles fragment registers), which puts both waves of a SIMD back into the same mixed stream
#define PS_FENCE() do { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0); } while (0)
    if (grp == 0) {
        if (nk > 0) { issue_b(0); issue_a(0, 0); }
    } else {
        if (nk > 0) issue_a(0, 1);
        if (nk > 1) issue_a(1, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PS_FENCE();
    if (grp == 0) {
        if (nk > 1) issue_b(1);
        read(0);
        PS_FENCE();
        for (int kt = 0; kt < nk; ++kt) {
            compute();
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // B of stage kt + 1 (issued one phase ago) has landed
            PS_FENCE();
            if (kt + 1 < nk) {
                if (kt + 2 < nk) issue_b(kt + 2);                         // stage kt: both groups have read it
                read(kt + 1);
            }
            PS_FENCE();
        }
    } else {
        PS_FENCE();
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 1 < nk) issue_a(kt + 1, 1);                          // own A half of the next stage: this group read that buffer last in read(kt - 1)
            if (kt + 2 < nk) issue_a(kt + 2, 0);                          // group 0's A half of the stage after: group 0 read that buffer in the previous phase
            read(kt);
            __builtin_amdgcn_sched_barrier(0);
            // everything older than this phase's pieces has landed: group 0's A half of stage kt + 1 (counted: the tail issues fewer pieces)
            if (kt + 2 < nk) { if (PH == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); }
            else if (kt + 1 < nk) { if (PH == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); }
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            PS_FENCE();
            compute();
            __builtin_amdgcn_sched_barrier(0);
            // ... and the own A half of stage kt + 1; the four pieces issued behind it (group 0's half of stage kt + 2) stay in flight
            if (kt + 2 < nk) { if (PH == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); }
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            PS_FENCE();
        }
    }
#undef PS_FENCE
    if (g.dbg & 1) return;
    // ---- epilogue: gemm_huge_kernel's (wave-private LDS slices over the dead stages, 64- or 32-row chunks, no block barriers)
    constexpr int WS = 68, CF = RF == 8 ? 4 : 2;
    float* clw = (float*)smem + wave * (64 * WS);
    EpiState es;
#pragma unroll
    for (int h = 0; h < RF / CF; ++h) {
#pragma unroll
        for (int i = 0; i < CF; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    clw[(i * 16 + (lane >> 4) * 4 + r) * WS + j * 16 + (lane & 15)] = acc[h * CF + i][j][r];
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        gemm_epilogue<CF * 16, 64, F, 8, WS>(g, clw, m0 + grp * (RF * 16) + h * (CF * 16), n0 + wn * 64, 0, es, (h == 0 ? 1 : 0) | (h == RF / CF - 1 ? 2 : 0));
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------------
// Ping-pong 256x256x32 weight-gradient kernel.  8 waves in two groups of four -- group g = wave >> 2 owns rows [128 g, 128 g + 128) of
// the tile, wave & 3 its 64-column strip -- so every SIMD hosts ONE wave of each group (waves w and w + 4 land on the
// same SIMD).  The groups run the same READ(t) / COMPUTE(t) sequence ONE barrier apart: while a group's waves issue
// their 16 v_mfma_f32_32x32x16_bf16 of k-tile t (pure register work, 512 cycles), the partner waves on the same SIMDs
// read the fragments of their next k-tile from LDS and issue the direct-to-LDS loads of the tile three ahead.  The
// fragment reads are therefore off the matrix pipe's critical path -- what the weight-gradient (TN) layout needs: both
// of its operands are contraction-strided and go through ds_read_b64_tr_b16, twice the LDS instructions of the
// K-contiguous layout (measured: the 2-phase TN kernel is LDS-ISSUE bound at ~600 TFLOP/s, half the NT rate).
// k-tiles of 32 in a ring of four 32 KB stages: a stage is refilled two barriers after its last read and has ~4 steps
// to land, waited for with a COUNTED vmcnt.
//   stage: [32 k][256 n] per operand, 512-byte k-rows, 32-byte chunk c of row k stored at c ^ skey(k).
// The same schedule on the K-contiguous (forward / input-gradient) layout was built in round 2 and only tied the 2-phase
// 256 x 256 kernel -- its 32-wide k-tiles are 64-byte row pieces, 50 instead of 75 GB/s per CU out of L2
// (profiles/r02_gemm_feed_ubench.md) -- and was removed in round 4 (profiles/r04_gemm_experiments.md).
// ------------------------------------------------------------------------------------------------------
#define PP_BK 32
#define PP_STAGE 32768
#define PP_NS 4
#define PP_LDS HUGE_LDS

// 32x32x16 operand fragment (32 rows/cols x 16 k) of a contraction-strided tile [k][256], 512-byte k-rows: byte offset of
// this lane's first transposing read inside the tile (k-rows k .. k+3); the second read (k+4 .. k+7) is 2048 bytes further
__device__ __forceinline__ int pp_frag_strided_off(int blk32, int ks2, int lane) {
    const int i = lane & 15, q = lane >> 4, r = i >> 2, c = i & 3;
    const int t16 = blk32 * 2 + (q & 1);
    const int k = ks2 * 16 + 8 * (q >> 1) + r;
    return k * 512 + ((t16 ^ skey(k)) << 5) + c * 8;
}
// ds_read_b64_tr_b16 as inline asm: the builtin makes hipcc drain EVERY outstanding direct-to-LDS load (s_waitcnt vmcnt(0))
// in front of the reads, which serialises the refill pipeline.  The destination is valid only after the caller's own
// s_waitcnt lgkmcnt(0) (+ sched_barrier) -- nothing may touch it before.
__device__ __forceinline__ s16x4 tr_read_async(unsigned lds_addr) {
    s16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(lds_addr));
    return v;
}
__device__ __forceinline__ s16x4 tr_read_async_2k(unsigned lds_addr) {
    s16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(v) : "v"(lds_addr));
    return v;
}
__device__ __forceinline__ bf16x8 join_frag(s16x4 lo, s16x4 hi) {
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = lo; u.s.b = hi;
    return u.v;
}

// TN refill piece as inline asm, scalar base + per-lane 32-bit offset (no per-piece VALU, 4 offset registers per wave in
// total).  Why asm: with the builtin hipcc knows an LDS-DMA is outstanding and drains it (s_waitcnt vmcnt(0)) in front of
// every ds_read_b64_tr_b16 -- the transposing read "may alias" -- which serialises the refill pipeline.  Hidden from its
// scoreboard, the loads are ordered by this kernel's own counted vmcnt + barriers only.
__device__ __forceinline__ void pp_dma_saddr(unsigned lds_dst, const void* sbase, unsigned voff) {
    unsigned keep_m0;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep_m0) : "v"(voff), "s"(lds_dst), "s"(sbase) : "memory");
}

__device__ __forceinline__ void pp_wait_tiles(int rem) {   // s_waitcnt vmcnt(4 * rem): `rem` younger k-tiles stay in flight
    if (rem >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (rem == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// walk: 0 = per-job XCD runs, n-fastest tiles (rounds 2-4); 1 = the caller has already placed `bid_in` (grouped launch: XCD runs over the
// WHOLE launch, so an XCD's ~27 co-resident blocks are consecutive tiles of ONE job and ONE K-slab) and the tiles of a slab are walked
// short-dimension-fastest: a run of L tiles then touches short + L / short operand panels instead of up to 2 L / long + long.
template <bool TN, unsigned F, int DBG = 0>
__device__ __forceinline__ void gemm_pp_body(const GemmArgs& g, int bid_in, int walk = 0) {
    static_assert(TN && F == EF_TNFLUSH && DBG == 0, "ping-pong kernel: weight-gradient layout only (the K-contiguous form was removed in round 4)");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wn = wave & 3;
    const int tiles_n = (g.N + 255) / 256, tiles_m = (g.M + BIG_BM - 1) / BIG_BM;
    const int nwg = tiles_m * tiles_n;
    int bid = bid_in;
    if (!(walk & 1)) {
        const int tot = nwg * g.splits;
        int q = tot >> 3, r = tot & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int split = bid / nwg;
    bid -= split * nwg;
    const bool m_fast = (walk & 2) && tiles_m < tiles_n;
    const int m0 = (m_fast ? bid % tiles_m : bid / tiles_n) * BIG_BM, n0 = (m_fast ? bid / tiles_m : bid % tiles_n) * 256;
    const int kbeg = split * g.k_per_split;
    const int kend = min(g.K, kbeg + g.k_per_split);
    const int nk = (kend - kbeg) / PP_BK;
    constexpr int D = PP_NS - 1;                           // prefetch distance in k-tiles

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    bf16x8 fa[4][2], fb[2][2];
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    int toa[4][2], tob[2][2];                              // TN: per-lane byte offsets of the first read of each fragment inside a stage
    if (TN) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
            for (int i = 0; i < 4; ++i) toa[i][s2] = pp_frag_strided_off(grp * 4 + i, s2, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) tob[j][s2] = 16384 + pp_frag_strided_off(wn * 2 + j, s2, lane);
        }
    }
    // TN: bias gradient = row sums of A^T (= column sums of dy), by the wn == 0 waves of the n0 == 0 blocks, on the VALU
    // from the A fragments they hold anyway (a ones-fragment MFMA would need 64 more accumulator registers per wave)
    const bool do_rowsum = TN && g.e.rowsum_a != nullptr && n0 == 0 && wn == 0;
    float rsum[4] = {0.f, 0.f, 0.f, 0.f};
    const float* keep = TN ? g.e.k_keep : nullptr;

    // TN refills: byte offset of this lane's 16 bytes of piece p relative to the first k-row of the tile (clamped columns)
    unsigned voff[4] = {0, 0, 0, 0};
    if (TN) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int tp = wave * 2 + (p & 1);
            const bool isb = p >= 2;
            const int krow = tp * 2 + (lane >> 5);
            const int ch = ((lane & 31) >> 1) ^ skey(krow);
            const int O = isb ? g.N : g.M;
            const int col = min((isb ? n0 : m0) + ch * 16 + (lane & 1) * 8, ((O + 7) & ~7) - 8);
            voff[p] = (unsigned)(((long)krow * (isb ? g.ldb : g.lda) + col) * 2);
        }
    }
    // piece p of k-tile tsrc into the stage of k-tile tdst (tdst == tsrc except for the phantom refills past the last tile)
    auto issue_piece = [&](int tdst, int tsrc, int p) {
        if constexpr (TN) {
            const int tp = wave * 2 + (p & 1);
            const bool isb = p >= 2;
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((tdst % PP_NS) * PP_STAGE + (isb ? 16384 : 0) + tp * 1024));
            const bf16_t* base = (isb ? g.B : g.A) + (long)(kbeg + tsrc * PP_BK) * (isb ? g.ldb : g.lda);
            pp_dma_saddr(dst, base, voff[p]);     // (non-temporal operand loads here were measured +0.9 ms per step: the dx GEMM of the main stream shares dy through the caches)
        }
    };
    auto issue = [&](int t) {
#pragma unroll
        for (int p = 0; p < 4; ++p) issue_piece(t, t, p);
    };
    // drop-path row skipping (TN): 0 = every contraction row of the k-tile belongs to a dropped sample, 1 = all kept,
    // 2 = the tile straddles a kept and a dropped sample (rows_per_group >= 32: at most one boundary, at row kb).
    // The keep flags of all samples sit in two 64-bit wave-uniform masks (one ballot each at kernel start) and the sample
    // of the current k-tile is tracked incrementally: no loads, no divisions in the loop.
    int kmode = 1;
    unsigned long long km0 = ~0ull, km1 = ~0ull;
    int cur_s = 0, nxt_b = 0x7fffffff;                     // sample of the next k-tile to read, first contraction row of the sample after it
    if (TN && keep) {
        const int ns = (g.K + g.e.k_rows_per_group - 1) / g.e.k_rows_per_group;
        km0 = __ballot(lane < ns ? keep[lane] != 0.f : true);
        km1 = __ballot(lane + 64 < ns ? keep[lane + 64] != 0.f : true);
        cur_s = kbeg / g.e.k_rows_per_group;
        nxt_b = (cur_s + 1) * g.e.k_rows_per_group;
    }
    auto kept = [&](int sidx) { return ((sidx < 64 ? km0 >> sidx : km1 >> (sidx - 64)) & 1ull) != 0; };
    auto read = [&](int t) {
        const char* st = smem + (t % PP_NS) * PP_STAGE;
        int kb = PP_BK; bool keep0 = true, keep1 = true;
        if (TN && keep) {
            const int k0 = kbeg + t * PP_BK;
            while (k0 >= nxt_b) { ++cur_s; nxt_b += g.e.k_rows_per_group; }
            kb = nxt_b - k0;
            keep0 = kept(cur_s);
            keep1 = kb < PP_BK ? kept(cur_s + 1) : keep0;
            kmode = (keep0 && keep1) ? 1 : (!keep0 && !keep1) ? 0 : 2;
            if (kmode == 0) return;
        }
        if constexpr (TN) {
#pragma unroll
            for (int s2 = 0; s2 < ((DBG & 2) ? (t == 0 ? 2 : 0) : 2); ++s2) {
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[j][s2] = join_frag(tr_read(st, tob[j][s2]), tr_read(st, tob[j][s2] + 2048));
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[i][s2] = join_frag(tr_read(st, toa[i][s2]), tr_read(st, toa[i][s2] + 2048));
            }
            if (__builtin_amdgcn_readfirstlane(kmode) == 2) {
                // rare (one k-tile per sample boundary): zero the dy rows of the dropped sample in the fragments; element e of
                // fa[.][s2] is contraction row 16 s2 + 8 (lane >> 5) + e
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const int kl = 16 * s2 + 8 * (lane >> 5);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        asm volatile("; straddling k-tile" : "+v"(fa[i][s2]));    // not speculatable: keeps the masking out of the common path
                        union { bf16x8 v; uint16_t h[8]; } u; u.v = fa[i][s2];
#pragma unroll
                        for (int e = 0; e < 8; ++e) if (!((kl + e) < kb ? keep0 : keep1)) u.h[e] = 0;
                        fa[i][s2] = u.v;
                    }
                }
            }
        }
    };
    int newest = -1;                                       // newest k-tile this wave has issued loads for
    // Every COMPUTE(t) issues the loads of k-tile t + D between its MFMAs (a direct-to-LDS load costs ~60 cycles of issue among
    // bare MFMAs, 100-185 next to the fragment reads of a READ segment) -- UNCONDITIONALLY, so that the 16-MFMA sequence stays
    // one basic block (a branch inside it, or a second copy of it, makes the 16-register accumulator tuples spill).  Past the
    // end of the contraction the loads re-fetch the last k-tile into a stage nobody reads any more (D tiles per block).
    auto compute = [&](int trefill) {
        const int tsrc = trefill < nk ? trefill : nk - 1;
        if (!(DBG & 1)) newest = trefill;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!(TN && kmode == 0) && !(DBG & 4)) {
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][s2], fb[j][s2], acc[i][j], 0, 0, 0);
                }
                if (!(DBG & 1) && (i & 1) == 0) issue_piece(trefill, tsrc, s2 * 2 + (i >> 1));
            }
        __builtin_amdgcn_s_setprio(0);
        if (TN && do_rowsum && kmode != 0) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    union { bf16x8 v; uint4 u; } u; u.v = fa[i][s2];
                    float f[8];
                    unpack8(u.u, f);
                    rsum[i] += ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
                }
        }
    };
    // before the barrier that precedes the first read of k-tile tn: this wave's pieces of it have landed
    auto wait_for = [&](int tn) {
        if (tn < nk) pp_wait_tiles(newest - tn);
    };

    // Stage of k-tile t is free once both groups have read it: after the barrier that ends step 2 t + 1.  Group 0 refills it
    // (with tile t + PP_NS) inside COMPUTE(t + 1) at step 2 t + 3, group 1 inside COMPUTE(t + 1) at step 2 t + 4.
    const int npro = nk < D ? nk : D;
    for (int t = 0; t < npro; ++t) issue(t);
    newest = npro - 1;
    pp_wait_tiles(npro - 1);
    __builtin_amdgcn_s_barrier();

    if (grp == 0) {
        if (nk > 0) read(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        for (int t = 0; t < nk; ++t) {
            compute(t + D);                                  // stage (t - 1) % PP_NS: tile t - 1 was last read at step 2 t - 1
            wait_for(t + 1);
            __builtin_amdgcn_s_barrier();
            if (t + 1 < nk) read(t + 1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the stage may be refilled after the next barrier
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
        }
    } else {
        __builtin_amdgcn_s_barrier();
        for (int t = 0; t < nk; ++t) {
            read(t);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            wait_for(t + 1);
            __builtin_amdgcn_s_barrier();
            compute(t + D);
            __builtin_amdgcn_s_barrier();
        }
    }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // phantom refills: the epilogue reuses the stages
    __builtin_amdgcn_s_barrier();
    if (TN && do_rowsum) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v = rsum[i] + __shfl_xor(rsum[i], 32, 64);
            const int row = m0 + grp * 128 + i * 32 + (lane & 31);
            if (lane < 32 && row < g.M) atomicAdd(g.e.rowsum_a + row, v * g.e.alpha);
        }
    }
    if constexpr (F == EF_TNFLUSH) {
        // weight-gradient flush: the tile goes through the block-wide fp32 staging in two 128-column halves
        float* cl = (float*)smem;
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            if ((wn >> 1) == h) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            cl[(grp * 128 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * CSTRIDE + (wn & 1) * 64 + j * 32 + (lane & 31)] = acc[i][j][r];
            }
            __syncthreads();
            gemm_epilogue<BIG_BM, 512, F>(g, cl, m0, n0 + h * 128, split);
            __syncthreads();
        }
    }
}

template <bool TN, unsigned F, int DBG = 0>
__global__ __launch_bounds__(512) void gemm_pp_kernel(GemmArgs g) { gemm_pp_body<TN, F, DBG>(g, (int)blockIdx.x); }

// GROUPED weight gradients (lav_gemm_tn_grouped): up to four independent C_j += A_j^T B_j products in ONE launch -- the four weight
// gradients of a Swin block / a fusion layer.  Launched one by one each of them needs 8-32 split-K parts to put ~128 workgroups on the
// machine (partial tiles through the fp32 workspace, a reduction pass each, k-loops of 15-40 steps); together their 26-108 tiles need 1-3
// parts.  Block b belongs to the job whose first block is the largest blk0 <= b; the job is selected by an if-chain over CONSTANT
// indices so that every copy of the body reads its GemmArgs straight from the kernel arguments (a run-time index would make the compiler
// copy the 1.6 KB table to scratch).
struct GemmGroup { int n; int walk; int blk0[4]; GemmArgs g[4]; };
template <bool TN, unsigned F>
__global__ __launch_bounds__(512) void gemm_pp_group_kernel(GemmGroup G) {
    int b = (int)blockIdx.x;
    if (G.walk & 1) {
        // hardware block b runs on XCD b % 8: give each XCD one contiguous run of the launch's (job, K-slab, tile) sequence
        const int tot = (int)gridDim.x;
        const int q = tot >> 3, r = tot & 7, xcd = b & 7, idx = b >> 3;
        b = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    if (G.n > 3 && b >= G.blk0[3]) gemm_pp_body<TN, F>(G.g[3], b - G.blk0[3], G.walk);
    else if (G.n > 2 && b >= G.blk0[2]) gemm_pp_body<TN, F>(G.g[2], b - G.blk0[2], G.walk);
    else if (G.n > 1 && b >= G.blk0[1]) gemm_pp_body<TN, F>(G.g[1], b - G.blk0[1], G.walk);
    else gemm_pp_body<TN, F>(G.g[0], b, G.walk);
}

// ---- split-K reduction: C[r][c] += sum_s ws[s][tile(r,c)][r % 128][c % 128] -------------------------------------
// 64 float4 outputs per block x 4 split lanes (each sums every 4th split, loads unrolled for memory parallelism),
// merged through LDS; one plain read-modify-write of C per output.
__device__ __forceinline__ void tn_reduce_body(const float* __restrict__ ws, int splits, int tiles, int tiles_n, int rpt, int M,
                                               int N, float* __restrict__ C, long ldc, int block, int assign) {
    __shared__ float4 part[4][64];
    const int n4 = N >> 2;
    const int o = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const long idx = (long)block * 64 + o;
    const bool valid = idx < (long)M * n4;
    const int row = valid ? (int)(idx / n4) : 0, col = valid ? (int)(idx % n4) * 4 : 0;
    const long off = ((long)(row / rpt) * tiles_n + col / BN) * (rpt * BN) + (row % rpt) * BN + (col % BN);   // rpt rows per tile
    const long stride = (long)tiles * (rpt * BN);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) {
        int sp = sl;
        for (; sp + 12 < splits; sp += 16) {
            const float4 v0 = *(const float4*)(ws + (long)sp * stride + off);
            const float4 v1 = *(const float4*)(ws + (long)(sp + 4) * stride + off);
            const float4 v2 = *(const float4*)(ws + (long)(sp + 8) * stride + off);
            const float4 v3 = *(const float4*)(ws + (long)(sp + 12) * stride + off);
            a.x += (v0.x + v1.x) + (v2.x + v3.x); a.y += (v0.y + v1.y) + (v2.y + v3.y);
            a.z += (v0.z + v1.z) + (v2.z + v3.z); a.w += (v0.w + v1.w) + (v2.w + v3.w);
        }
        for (; sp < splits; sp += 4) {
            const float4 v = *(const float4*)(ws + (long)sp * stride + off);
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
    }
    part[sl][o] = a;
    __syncthreads();
    if (sl == 0 && valid) {
        const float4 b = part[1][o], c = part[2][o], d = part[3][o];
        float4* p = (float4*)(C + (long)row * ldc + col);
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!assign) r = *p;
        r.x += (a.x + b.x) + (c.x + d.x); r.y += (a.y + b.y) + (c.y + d.y);
        r.z += (a.z + b.z) + (c.z + d.z); r.w += (a.w + b.w) + (c.w + d.w);
        *p = r;
    }
}

__global__ __launch_bounds__(256) void tn_reduce_kernel(const float* __restrict__ ws, int splits, int tiles, int tiles_n, int rpt, int M,
                                                       int N, float* __restrict__ C, long ldc, int assign) {
    tn_reduce_body(ws, splits, tiles, tiles_n, rpt, M, N, C, ldc, (int)blockIdx.x, assign);
}
// the reductions of a grouped weight-gradient launch (lav_gemm_tn_grouped) as one launch
struct TnReduceJob { const float* ws; float* C; long ldc; int splits, tiles, tiles_n, rpt, M, N, blk0, assign; };
struct TnReduceGroup { int n; TnReduceJob j[4]; };
__global__ __launch_bounds__(256) void tn_reduce_group_kernel(TnReduceGroup G) {
    const int b = (int)blockIdx.x;
    int p = 0;
    if (G.n > 3 && b >= G.j[3].blk0) p = 3; else if (G.n > 2 && b >= G.j[2].blk0) p = 2; else if (G.n > 1 && b >= G.j[1].blk0) p = 1;
    // constant indices: the job is read from the kernel arguments (no scratch copy of the table)
    if (p == 3) tn_reduce_body(G.j[3].ws, G.j[3].splits, G.j[3].tiles, G.j[3].tiles_n, G.j[3].rpt, G.j[3].M, G.j[3].N, G.j[3].C, G.j[3].ldc, b - G.j[3].blk0, G.j[3].assign);
    else if (p == 2) tn_reduce_body(G.j[2].ws, G.j[2].splits, G.j[2].tiles, G.j[2].tiles_n, G.j[2].rpt, G.j[2].M, G.j[2].N, G.j[2].C, G.j[2].ldc, b - G.j[2].blk0, G.j[2].assign);
    else if (p == 1) tn_reduce_body(G.j[1].ws, G.j[1].splits, G.j[1].tiles, G.j[1].tiles_n, G.j[1].rpt, G.j[1].M, G.j[1].N, G.j[1].C, G.j[1].ldc, b - G.j[1].blk0, G.j[1].assign);
    else tn_reduce_body(G.j[0].ws, G.j[0].splits, G.j[0].tiles, G.j[0].tiles_n, G.j[0].rpt, G.j[0].M, G.j[0].N, G.j[0].C, G.j[0].ldc, b, G.j[0].assign);
}

// split-K of a forward / input-gradient GEMM (bf16 output, no epilogue): C = bf16(sum_s ws[s]); 8 columns per thread
__global__ __launch_bounds__(256) void splitk_reduce_bf16_kernel(const float* __restrict__ ws, int splits, int tiles, int tiles_n, int rpt,
                                                                int M, int N, bf16_t* __restrict__ C, long ldc) {
    const int n8 = N >> 3;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)M * n8) return;
    const int row = (int)(idx / n8), col = (int)(idx % n8) * 8;
    const long off = ((long)(row / rpt) * tiles_n + col / BN) * (rpt * BN) + (row % rpt) * BN + (col % BN);
    const long stride = (long)tiles * (rpt * BN);
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int sp = 0; sp < splits; ++sp) {
        const float4 a = *(const float4*)(ws + (long)sp * stride + off), b = *(const float4*)(ws + (long)sp * stride + off + 4);
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
    }
    *(uint4*)(C + (long)row * ldc + col) = pack8(v);
}

// =================================================================================================================================
// Host side: the process-wide switches, the route plan (pure: the CPU tests call it through lav_gemm_plan), the kernel table and the entries.
// =================================================================================================================================

// split-K partial tiles live in the stream's LAV_WS_SPLITK workspace (runtime.cpp: registered by the caller with lav_set_workspace, or one internal
// allocation per stream).  Calls on the SAME stream are ordered, so they share it.
static float* splitk_workspace(void* stream, size_t bytes) { return (float*)lav_ws_get(stream, LAV_WS_SPLITK, bytes, nullptr); }

// ---- switches: read from the environment once, when the library is loaded; lav_gemm_select changes the numbered ones at run time ------------
struct GemmSwitches {
    int tn_kind;     // LAV_GEMM_TN_KIND: 0 = 128x128 weight-gradient tiles only, 1 = at most 256x128, default = largest tile that fits
    int pp_tn;       // LAV_GEMM_PP_TN (select 2): ping-pong kernel for the 256x256 weight-gradient tiles
    int dbg;         // LAV_GEMM_DBG (select 5): GemmArgs.dbg of the 256x256 kernel (timing only, wrong results)
    // tile walk of the 256x256 K-contiguous kernel: column groups of 4 tiles when the output is >= 8 tiles wide (an XCD's 32 resident
    // tiles then form an 8 x 4 block: 12 operand panels in its L2 instead of 15 for 2.7 rows x 12 columns; measured +8-12 % on the
    // 45120 x 3072 x 768 GEMMs and on 8192^3, nothing on narrower outputs).  0 restores n-fastest, other values force G, < 0 = that rule.
    int group_n;     // LAV_GEMM_GROUP_N (select 6)
    int h192;        // LAV_GEMM_H192 (select 7): 192-row tiles for outputs that under-fill the last round of 256-row tiles
    int h192l;       // LAV_GEMM_H192L (select 9): 192-row tiles: two loader waves issue the operand DMA (0 = off)
    int ps;          // LAV_GEMM_PS (select 11): phase-shifted kernel instead of gemm_huge (bit 0) / gemm_h192l (bit 1) for the specialised layout-0 epilogues (round 6: -2.0 ms per cfg2 step)
    int tn_min_m;    // LAV_GEMM_TN_MINM (select 12): fewest output rows that take the 256-row weight-gradient tiles (outputs with 160 ... 255 rows, Swin-L stage 0: C = 192,
                     // leave a quarter of the tile idle and are still well ahead of the 128 x 128 kernel; 256 restores the old threshold)
    int tn_group;    // LAV_GEMM_TN_GROUP (select 13): 0 = lav_gemm_tn_grouped runs its jobs one by one
    int nt_stores;   // LAV_NT_STORES: 1: GELU' stored non-temporally, 4: and loaded non-temporally by the gradient epilogue (73.30 -> 73.12 ms per step, two interleaved pairs)
    // workgroups the split-K policy aims a weight-gradient launch at (tn_splits / tn_group_splits; sweeps: profiles/r04_gemm_experiments.md section 8,
    // profiles/r04_late_experiments.md section 11)
    int tn_blocks;               // LAV_TN_BLOCKS: one weight-gradient GEMM on the large tiles
    int tn_group_blocks;         // LAV_TN_GROUP_BLOCKS: a grouped launch
    int tn_group_blocks_wide;    // LAV_TN_GROUP_BLOCKS_WIDE: a grouped launch of >= 96 tiles (the fusion layers); default = tn_group_blocks
};
static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
static GemmSwitches gemm_sw = {env_int("LAV_GEMM_TN_KIND", -1), env_int("LAV_GEMM_PP_TN", 1) != 0, env_int("LAV_GEMM_DBG", 0), env_int("LAV_GEMM_GROUP_N", -1),
                               env_int("LAV_GEMM_H192", 1), env_int("LAV_GEMM_H192L", 1), env_int("LAV_GEMM_PS", 3), env_int("LAV_GEMM_TN_MINM", 160),
                               env_int("LAV_GEMM_TN_GROUP", 1) != 0, env_int("LAV_NT_STORES", 5), env_int("LAV_TN_BLOCKS", 128),
                               env_int("LAV_TN_GROUP_BLOCKS", 192), env_int("LAV_TN_GROUP_BLOCKS_WIDE", env_int("LAV_TN_GROUP_BLOCKS", 192))};
// probe hook (within-process A/B): which = 2 pp_tn, 5 dbg, 6 group_n, 7 h192, 9 h192l, 11 ps, 12 tn_min_m, 13 tn_group; returns the old value, -1 for an unknown id
extern "C" int lav_gemm_select(int which, int value) {
    int* const p = which == 2 ? &gemm_sw.pp_tn : which == 5 ? &gemm_sw.dbg : which == 6 ? &gemm_sw.group_n : which == 7 ? &gemm_sw.h192 :
                   which == 9 ? &gemm_sw.h192l : which == 11 ? &gemm_sw.ps : which == 12 ? &gemm_sw.tn_min_m : which == 13 ? &gemm_sw.tn_group : nullptr;
    if (!p) return -1;
    const int old = *p;
    *p = which == 2 || which == 13 ? value != 0 : value;
    return old;
}

// ---- kernel table: every instantiation the plan can name, its launch constants, and whether its dynamic-LDS limit has been raised yet -------
constexpr unsigned S_B = EF_BIAS, S_BG = EF_BIAS | EF_ACT, S_GC = EF_GIN | EF_RSCALE | EF_COLSUM, S_BDR = EF_BIAS | EF_DROP | EF_RSCALE | EF_RES,
                   S_BDRO = S_BDR | EF_O32;
constexpr int FI_ALL = 5;                                    // feature-set index: S_B, S_BG, S_GC, S_BDR, S_BDRO, EF_ALL (the generic code)
enum GemmKernelId : int {
    GK_SMALL = 0,                                            // gemm_kernel: + layout (0 NT, 1 NN, 2 TN with the generic epilogue)
    GK_PS256 = GK_SMALL + 3,                                 // + feature index (specialised sets only)
    GK_HUGE = GK_PS256 + 5,                                  // + 2 * feature index + layout
    GK_PS192 = GK_HUGE + 12,                                 // + feature index (specialised sets only)
    GK_H192 = GK_PS192 + 5,                                  // + 3 * feature index (specialised sets only) + {0: loader-wave form (NT), 1: NT, 2: NN}
    GK_BIG = GK_H192 + 15,                                   // + 2 * feature index + layout
    GK_PP_TN = GK_BIG + 12, GK_HUGE_TN, GK_BIG_TN, GK_SMALL_TN,          // weight gradients with the flush epilogue
    GK_PP_GROUP, GK_TN_REDUCE, GK_TN_REDUCE_GROUP, GK_SPLITK_REDUCE, GK_COUNT
};
struct GemmKernel { const void* fn; const char* name; int threads, lds; bool attr_done; };
template <bool AKC, bool BKC, int KG, unsigned F = EF_ALL> static GemmKernel k_small() { return {(const void*)gemm_kernel<AKC, BKC, KG, F>, "gemm_kernel", NT_ * KG, KG == 1 ? GEMM_LDS_BYTES : 131072}; }
template <bool AKC, bool BKC, unsigned F> static GemmKernel k_big() { return {(const void*)gemm_big_kernel<AKC, BKC, F>, "gemm_big_kernel", 512, BIG_LDS}; }
template <bool AKC, bool BKC, unsigned F> static GemmKernel k_huge() { return {(const void*)gemm_huge_kernel<AKC, BKC, F>, "gemm_huge_kernel", 512, HUGE_LDS}; }
template <bool BKC, unsigned F> static GemmKernel k_h192() { return {(const void*)gemm_h192_kernel<true, BKC, F>, "gemm_h192_kernel", 512, HUGE_LDS}; }
template <unsigned F> static GemmKernel k_h192l() { return {(const void*)gemm_h192l_kernel<true, true, F>, "gemm_h192l_kernel", 640, HUGE_LDS}; }
template <unsigned F, int RF> static GemmKernel k_ps() { return {(const void*)gemm_ps_kernel<F, RF>, "gemm_ps_kernel", 512, HUGE_LDS}; }
static GemmKernel gemm_kernels[] = {
    k_small<true, true, 1>(), k_small<true, false, 1>(), k_small<false, false, 2>(),
    k_ps<S_B, 8>(), k_ps<S_BG, 8>(), k_ps<S_GC, 8>(), k_ps<S_BDR, 8>(), k_ps<S_BDRO, 8>(),
    k_huge<true, true, S_B>(), k_huge<true, false, S_B>(), k_huge<true, true, S_BG>(), k_huge<true, false, S_BG>(),
    k_huge<true, true, S_GC>(), k_huge<true, false, S_GC>(), k_huge<true, true, S_BDR>(), k_huge<true, false, S_BDR>(),
    k_huge<true, true, S_BDRO>(), k_huge<true, false, S_BDRO>(), k_huge<true, true, EF_ALL>(), k_huge<true, false, EF_ALL>(),
    k_ps<S_B, 6>(), k_ps<S_BG, 6>(), k_ps<S_GC, 6>(), k_ps<S_BDR, 6>(), k_ps<S_BDRO, 6>(),
    k_h192l<S_B>(), k_h192<true, S_B>(), k_h192<false, S_B>(), k_h192l<S_BG>(), k_h192<true, S_BG>(), k_h192<false, S_BG>(),
    k_h192l<S_GC>(), k_h192<true, S_GC>(), k_h192<false, S_GC>(), k_h192l<S_BDR>(), k_h192<true, S_BDR>(), k_h192<false, S_BDR>(),
    k_h192l<S_BDRO>(), k_h192<true, S_BDRO>(), k_h192<false, S_BDRO>(),
    k_big<true, true, S_B>(), k_big<true, false, S_B>(), k_big<true, true, S_BG>(), k_big<true, false, S_BG>(),
    k_big<true, true, S_GC>(), k_big<true, false, S_GC>(), k_big<true, true, S_BDR>(), k_big<true, false, S_BDR>(),
    k_big<true, true, S_BDRO>(), k_big<true, false, S_BDRO>(), k_big<true, true, EF_ALL>(), k_big<true, false, EF_ALL>(),
    {(const void*)gemm_pp_kernel<true, EF_TNFLUSH>, "gemm_pp_kernel", 512, PP_LDS},
    k_huge<false, false, EF_TNFLUSH>(), k_big<false, false, EF_TNFLUSH>(), k_small<false, false, 2, EF_TNFLUSH>(),
    {(const void*)gemm_pp_group_kernel<true, EF_TNFLUSH>, "gemm_pp_group_kernel", 512, PP_LDS},
    {(const void*)tn_reduce_kernel, "tn_reduce_kernel", 256, 0},
    {(const void*)tn_reduce_group_kernel, "tn_reduce_group_kernel", 256, 0},
    {(const void*)splitk_reduce_bf16_kernel, "splitk_reduce_bf16_kernel", 256, 0},
};
static_assert(sizeof(gemm_kernels) / sizeof(gemm_kernels[0]) == GK_COUNT, "gemm_kernels must hold one row per GemmKernelId");

// one launch: which kernel, how many blocks, and the output tile it works in (what lav_gemm_plan reports); kern < 0 = no launch
struct GemmLaunch { int kern; unsigned grid; int tile_m, tile_n; };
static void gemm_launch(const GemmLaunch& l, hipStream_t s, void** args) {
    GemmKernel& k = gemm_kernels[l.kern];
    if (k.lds && !k.attr_done) {
        hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds);
        (void)hipGetLastError();
        k.attr_done = true;
    }
    hipLaunchKernel(k.fn, dim3(l.grid), dim3(k.threads), args, k.lds, s);
}

// ---- route plan -------------------------------------------------------------------------------------------------------------------------
// One part = one GemmArgs: a GEMM launch over contraction rows [k_off, k_off + K) and, with a workspace split-K, its reduction.  A call is one
// part, or two for a ragged long weight-gradient contraction.  Everything the route fixes in GemmArgs is spelled out here, zeros included.
struct GemmPart {
    GemmLaunch gemm, reduce;
    int k_off, K;
    int N, nb_rows;                      // after the c_pad_writable rounding
    int k_per_split, splits, group_n, dbg, owner, assign;
    int ws_tiles, rpt;                   // workspace tiles per split and their rows; the reduction's tiles_n is ceil(N / BN)
    size_t ws_bytes;                     // > 0: the part needs this much split-K workspace
};
enum GemmPlanError { GP_OK = 0, GP_E_ROWMAP, GP_E_ASSIGN_SPLITK };
struct GemmPlan { int err, n_parts; GemmPart part[2]; };

// epilogue feature mask of a call -> index of the smallest instantiated superset
static int gemm_feature_index(int N, const lav_gemm_epilogue& e) {
    unsigned fm = 0;
    if (e.bias) fm |= EF_BIAS;
    if (e.act == 1 && (!e.preact || e.preact_is_grad)) fm |= EF_ACT;
    else if (e.act != 0 || e.preact) fm |= EF_GENERIC;
    if (e.gelu_in) fm |= e.gelu_in_is_grad ? EF_GIN : EF_GENERIC;
    if (e.dropout_p > 0.f) fm |= EF_DROP;
    if (e.row_scale) fm |= EF_RSCALE;
    if (e.residual) fm |= EF_RES;
    if (e.colsum) fm |= EF_COLSUM;
    if (e.out_mode == 1 || e.out_mode == 3) fm |= EF_O32;           // EF_O32 = 'not a bf16 store': fp32 or fp16 rows, told apart at run time
    if (e.out_mode == 2 || (N % 8) != 0) fm |= EF_GENERIC;
    return !(fm & ~S_B) ? 0 : !(fm & ~S_BG) ? 1 : !(fm & ~S_GC) ? 2 : !(fm & ~S_BDR) ? 3 : ((fm & EF_O32) && !(fm & ~S_BDRO)) ? 4 : FI_ALL;
}
// a plain weight-gradient flush: fp32 accumulate, nothing else in the epilogue (alpha, rowsum_a and k_keep are allowed)
static bool tn_plain(const lav_gemm_epilogue& e) {
    return e.out_mode == 2 && !e.bias && !e.act && !e.preact && !e.gelu_in && e.dropout_p <= 0.f && !e.row_scale && !e.residual && !e.colsum;
}
// rows enough for the 256-row weight-gradient tiles (192 x 768: 324 -> 198 us; 192 x 192: 112 -> 124 us, stays on the small kernel)
static bool tn_rows_enough(int M, int N, const GemmSwitches& sw) { return M >= (N >= 512 ? sw.tn_min_m : (sw.tn_min_m > 256 ? sw.tn_min_m : 256)); }
// fits the ping-pong weight-gradient kernel: 256 x 256 tiles, k-tiles of 32, drop-path groups of at least keep_rows rows and at most 128 of them
static bool tn_pp_fits(int M, int N, int K, const void* k_keep, int k_rows_per_group, int keep_rows, const GemmSwitches& sw) {
    return sw.pp_tn && sw.tn_kind != 0 && sw.tn_kind != 1 && tn_rows_enough(M, N, sw) && (N % 256) == 0 && (K % PP_BK) == 0 &&
           (!k_keep || (k_rows_per_group >= keep_rows && (K + k_rows_per_group - 1) / k_rows_per_group <= 128));
}
// the weight-gradient tile of a plain flush over contraction K: 0 = 128 x 128 (two-group kernel), 1 = 256 x 128, 2 = 256 x 256
static int tn_tile_kind(int M, int N, int K, const void* k_keep, int k_rows_per_group, const GemmSwitches& sw) {
    if ((K % BKT) == 0 && tn_rows_enough(M, N, sw) && (!k_keep || k_rows_per_group >= BKT))
        return sw.tn_kind == 0 ? 0 : (N % 256) == 0 && sw.tn_kind != 1 ? 2 : 1;
    // contraction lengths that are multiples of 32 but not of 64 (Swin stage 3: 7840 token rows): the ping-pong kernel walks k-tiles of 32
    // (k_per_split is a multiple of 64, so only the last split ends on a 32-boundary) -- before round 4 these fell to the 128 x 128 kernel
    return (K % BKT) != 0 && tn_pp_fits(M, N, K, k_keep, k_rows_per_group, BKT, sw) ? 2 : 0;
}
// a long weight-gradient contraction without drop-path rows on an output with rows enough: a K that is no multiple of the k-tile is split off (gemm_plan)
static bool tn_long_k(int M, int N, int K, bool keep, const GemmSwitches& sw) { return !keep && tn_rows_enough(M, N, sw) && K >= 2048 && sw.tn_kind != 0; }
// a workspace split-K of layouts 0 / 1 on the 256 x 256 tiles
static bool nn_sk_huge(int M, int N, int K) { return (K % BKT) == 0 && M >= BIG_BM && (N % 256) == 0; }
static int gemm_group_n(int N, const GemmSwitches& sw) {
    const int tn = N / 256;
    return sw.group_n >= 0 ? sw.group_n : (tn >= 8 && tn % 4 == 0 ? 4 : 0);
}

static GemmPlanError gemm_plan_part(GemmPart& q, int layout, int M, int N, int k_off, int K, long lda, long ldb, long ldc, const lav_gemm_epilogue& e,
                                    bool assign, int splits, const GemmSwitches& sw) {
    const int kps = ((K + splits - 1) / splits + BKT - 1) / BKT * BKT;          // a multiple of BKT, and so of PP_BK
    splits = (K + kps - 1) / kps;
    q.gemm = {-1, 0, 0, 0}; q.reduce = {-1, 0, 0, 0};
    q.k_off = k_off; q.K = K; q.N = N; q.nb_rows = 0;
    q.k_per_split = kps; q.splits = splits; q.group_n = 0; q.dbg = 0; q.owner = 0; q.assign = assign;
    q.ws_tiles = 0; q.rpt = 0; q.ws_bytes = 0;
    // ragged N whose padding columns the caller lets us overwrite (the 30522-wide vocabulary projection into its 30528-wide logits
    // buffer): run as N rounded up to 8 so that the 16-byte-chunk epilogues apply (the generic one was 566 vs 256 us for the vendor
    // library on 5120 x 30522 x 768); B rows and bias entries past the real N are never read
    if (e.c_pad_writable && (N % 8) != 0 && layout == 0 && splits == 1 && (K % BKT) == 0 && M >= 2048 && e.out_mode == 0 &&
        ldc >= (long)((N + 7) / 8 * 8) && !e.colsum && !e.preact && !e.gelu_in && !e.residual && !e.a_rowmap) {
        q.nb_rows = N;
        q.N = N = (N + 7) / 8 * 8;
    }
    const bool big = layout != 2 && splits == 1 && (K % BKT) == 0 && M >= 2048;
    const int fi = gemm_feature_index(N, e);
    const bool small32 = (long)M * lda * 2 < (1L << 31) && (long)N * ldb * 2 < (1L << 31);       // both operands below 2 GiB: what the phase-shifted kernels address
    // pick the tile by estimated machine fill: tiles / (rounds * resident slots), weighted by the tile's own efficiency
    auto fill = [](long tiles, long slots, double w) { return w * (double)tiles / (double)(((tiles + slots - 1) / slots) * slots); };
    const long t_small = (long)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    const long t_big = (long)((M + BIG_BM - 1) / BIG_BM) * ((N + BN - 1) / BN);
    const long t_huge = (long)((M + BIG_BM - 1) / BIG_BM) * (N / 256);
    constexpr double w_big = 0.80;                            // measured best once the dW stream fills partial rounds (0.88 before)
    const double f_small = fill(t_small, 512, 0.80), f_big = fill(t_big, 256, w_big);
    const double f_huge = ((N % 256) == 0 && !q.nb_rows) ? fill(t_huge, 256, 1.0) : 0.0;
    // 192-row tiles where they fill the machine better (narrow outputs: N = 768 at M = 45120 is 2.07 rounds of 256-row tiles)
    const long t_h192 = (long)((M + 191) / 192) * (N / 256);
    const double f_h192 = ((N % 256) == 0 && fi != FI_ALL && sw.h192 && !q.nb_rows) ? fill(t_h192, 256, 0.97) : 0.0;
    if (e.a_rowmap) {                                        // pair-expanded A rows: the 256 x 256 kernel reads them through the map
        if (!(layout == 0 && splits == 1 && (N % 256) == 0 && (K % BKT) == 0)) return GP_E_ROWMAP;
        q.k_per_split = K;
        q.group_n = gemm_group_n(N, sw); q.dbg = 0;
        // (M bounds the mapped rows' source too: the map indexes rows of A below the caller's source row count <= M)
        q.gemm = {(sw.ps & 1) && fi != FI_ALL && small32 ? GK_PS256 + fi : GK_HUGE + 2 * fi, (unsigned)t_huge, 256, 256};
        return GP_OK;
    }
    if (big && f_h192 > f_huge + 0.02 && f_h192 >= f_big && f_h192 >= f_small) {
        q.k_per_split = K;
        q.group_n = 0; q.dbg = sw.dbg;
        q.gemm = {(sw.ps & 2) && layout == 0 && small32 ? GK_PS192 + fi : GK_H192 + 3 * fi + (layout == 0 ? (sw.h192l ? 0 : 1) : 2), (unsigned)t_h192, 192, 256};
        return GP_OK;
    }
    if (big && f_huge >= f_big && f_huge >= f_small) {
        q.k_per_split = K;
        q.group_n = gemm_group_n(N, sw); q.dbg = sw.dbg;
        q.gemm = {(sw.ps & 1) && layout == 0 && fi != FI_ALL && small32 ? GK_PS256 + fi : GK_HUGE + 2 * fi + layout, (unsigned)t_huge, 256, 256};
        return GP_OK;
    }
    if (big && (f_big >= f_small || q.nb_rows)) {
        q.k_per_split = K;
        q.group_n = 0; q.dbg = 0;
        q.gemm = {GK_BIG + 2 * fi + layout, (unsigned)t_big, 256, 128};
        return GP_OK;
    }
    if (layout != 2) {
        const bool sk = splits > 1 && e.out_mode == 0;       // under-filled long-K problem (vocabulary contraction): workspace split-K
        const bool sk_huge = sk && nn_sk_huge(M, N, K);
        q.group_n = 0; q.dbg = 0;
        if (sk_huge) q.gemm = {GK_HUGE + 2 * FI_ALL + layout, (unsigned)(t_huge * splits), 256, 256};
        else q.gemm = {GK_SMALL + layout, (unsigned)(t_small * splits), 128, 128};
        if (sk) {
            q.rpt = sk_huge ? BIG_BM : BM;
            q.ws_tiles = ((M + q.rpt - 1) / q.rpt) * ((N + BN - 1) / BN);
            q.ws_bytes = (size_t)splits * q.ws_tiles * q.rpt * BN * sizeof(float);
            q.reduce = {GK_SPLITK_REDUCE, (unsigned)(((long)M * (N / 8) + 255) / 256), q.gemm.tile_m, q.gemm.tile_n};
        }
        return GP_OK;
    }
    // ---- weight gradients ---------------------------------------------------------------------------------------------------------------
    // flush (out_mode 2): one block per output tile -> plain read-modify-write; split-K -> private partial tiles in a
    // workspace + one reduction pass.  fp32 atomics only remain for ragged N.
    const bool plain = tn_plain(e);
    const int kind = plain ? tn_tile_kind(M, N, K, e.k_keep, e.k_rows_per_group, sw) : 0;
    q.group_n = 0; q.dbg = 0;
    q.rpt = kind ? BIG_BM : BM;
    const int ws_tiles = ((M + q.rpt - 1) / q.rpt) * ((N + BN - 1) / BN);
    if (e.out_mode == 2) {
        if (splits == 1) q.owner = 1;
        else if ((N % 4) == 0 && (ldc % 4) == 0) {
            q.ws_tiles = ws_tiles;
            q.ws_bytes = (size_t)splits * ws_tiles * q.rpt * BN * sizeof(float);
            q.reduce = {GK_TN_REDUCE, (unsigned)(((long)M * (N / 4) + 63) / 64), q.rpt, BN};
        }
        if (assign && !q.owner && !q.ws_bytes) return GP_E_ASSIGN_SPLITK;
    }
    if (kind == 2) q.gemm = {tn_pp_fits(M, N, K, e.k_keep, e.k_rows_per_group, PP_BK, sw) ? GK_PP_TN : GK_HUGE_TN, (unsigned)(t_huge * splits), 256, 256};
    else if (kind == 1) q.gemm = {GK_BIG_TN, (unsigned)(ws_tiles * splits), 256, 128};
    else q.gemm = {plain ? GK_SMALL_TN : GK_SMALL + 2, (unsigned)(t_small * splits), 128, 128};
    return GP_OK;
}

// The route of one (validated) lav_gemm_bf16 call.  Pure: no HIP call, no workspace, no process state -- the switches come in as an argument.
// e is the call's epilogue with the defaults filled in (gemm_check_args); its pointers are only tested for presence.
static GemmPlan gemm_plan(int layout, int M, int N, int K, long lda, long ldb, long ldc, const lav_gemm_epilogue& e, int splits, const GemmSwitches& sw) {
    GemmPlan p;
    // A long weight-gradient contraction that is not a multiple of the k-tile (the fusion encoder's token rows n * L: 30280 at cfg4, 33840 at the
    // reference's shipped batch of 24) used to drop the whole weight gradient onto the 128 x 128 kernel (18 ms per cfg4 step on the
    // weight-gradient stream).  Split it instead: the first K - K % 64 rows on the large-tile kernels (with the call's split factor, clamped to what
    // the whole K allows), the < 64-row tail on the small one; both accumulate into C on the same stream (alpha, rowsum_a apply to both parts);
    // the first part assigns when the call does, the tail always accumulates.
    if (layout == 2 && tn_plain(e) && tn_long_k(M, N, K, e.k_keep != nullptr, sw) && (K % PP_BK) != 0) {
        const int K0 = K / BKT * BKT, kps = ((K + splits - 1) / splits + BKT - 1) / BKT * BKT;
        p.n_parts = 2;
        p.err = gemm_plan_part(p.part[0], layout, M, N, 0, K0, lda, ldb, ldc, e, e.assign != 0, (K + kps - 1) / kps, sw);
        if (!p.err) p.err = gemm_plan_part(p.part[1], layout, M, N, K0, K - K0, lda, ldb, ldc, e, false, 1, sw);
        return p;
    }
    p.n_parts = 1;
    p.err = gemm_plan_part(p.part[0], layout, M, N, 0, K, lda, ldb, ldc, e, e.assign != 0, splits, sw);
    return p;
}

// ---- split-K policy ---------------------------------------------------------------------------------------------------------------------
// The factor a caller should pass as `splits` (the caller owns the workspace, so it has to know the factor before the call).  Pure, like the plan,
// and written with the plan's predicates and tile constants: a threshold that moves there moves the factor with it.
constexpr int TN_SPLIT_MIN_K = 256;                          // a weight-gradient split is worth at least this many contraction rows
static int clamp_splits(int want, int most) { return want < most ? (want > 1 ? want : 1) : (most > 1 ? most : 1); }

// One weight-gradient call, matched to the tile the plan gives it.  Measured on MI355X (tools/tn_probe.py): every tile holds one block per CU and is
// fastest IN ISOLATION when tiles x splits lands just under 256; in the step these launches share the chip with the input-gradient chain of the
// compute stream, which is the critical path, and about half the CUs (tn_blocks) is the better target (fewer partial tiles through the workspace,
// CUs left to the other stream).  keep: the call has drop-path k_keep rows; their row groups are taken to fit the large tiles (the shipped ones
// do: whole samples), since whoever asks does not know the group size yet.
static int tn_splits(int M, int N, int K, bool keep, const GemmSwitches& sw) {
    int kind = tn_tile_kind(M, N, K, nullptr, 1, sw);
    // a ragged long contraction: the factor is for the first part, K rounded down to the k-tile (gemm_plan).  This also holds for K % 64 == 32 on an
    // output the ping-pong kernel does not take (N % 256 != 0), which the plan does NOT split off and runs on 128 x 128 tiles: the factor such a
    // shape had before the policy moved here, kept as it was (no shipped shape is one)
    if (!kind && tn_long_k(M, N, K, keep, sw)) kind = tn_tile_kind(M, N, K / BKT * BKT, nullptr, 1, sw);
    if (kind) {
        const int tiles = ((M + BIG_BM - 1) / BIG_BM) * (kind == 2 ? N / 256 : (N + BN - 1) / BN);
        return clamp_splits(tiles <= sw.tn_blocks ? sw.tn_blocks / tiles : 1, K / TN_SPLIT_MIN_K);
    }
    const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);                 // 128 x 128 tiles: two blocks per CU
    if (tiles >= 200) return 1;
    return clamp_splits(tiles > 128 ? 5 : 256 / tiles, (K + TN_SPLIT_MIN_K - 1) / TN_SPLIT_MIN_K);
}
// A forward / input-gradient call whose output is too small to fill the chip while K is long (d_hidden = dlogits . W_dec: K = vocabulary)
static int nn_splits(int M, int N, int K) {
    if (K < 4096 || (N % 8) != 0) return 1;
    if (nn_sk_huge(M, N, K)) {                               // 256 x 256 tiles: one block per CU
        const int tiles = ((M + BIG_BM - 1) / BIG_BM) * (N / 256);
        return tiles < 128 ? clamp_splits(256 / tiles, K / 1024) : 1;
    }
    const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    return tiles < 256 ? clamp_splits(512 / tiles, K / 1024) : 1;
}

// ---- entries ----------------------------------------------------------------------------------------------------------------------------
// the argument checks of lav_gemm_bf16 (lav_gemm_plan runs them without operand pointers); fills e and splits with the defaults applied
static int gemm_check_args(int layout, int M, int N, int K, bool with_operands, const void* A, long lda, const void* B, long ldb, const void* C, long ldc,
                           const lav_gemm_epilogue* epi, lav_gemm_epilogue& e, int& splits) {
    LAV_REQUIRE(M > 0 && N > 0 && K > 0, "lav_gemm_bf16: empty problem M=%d N=%d K=%d", M, N, K);
    LAV_REQUIRE(layout >= 0 && layout <= 2, "lav_gemm_bf16: bad layout %d", layout);
    LAV_REQUIRE(!with_operands || (A && B && C), "lav_gemm_bf16: null operand");
    LAV_REQUIRE((lda % 8) == 0 && (ldb % 8) == 0, "lav_gemm_bf16: lda/ldb must be multiples of 8 (16-byte rows)");
    LAV_REQUIRE(!with_operands || (((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0 && ((uintptr_t)C % 16) == 0),
                "lav_gemm_bf16: operands must be 16-byte aligned");
    if (epi) e = *epi; else { memset(&e, 0, sizeof(e)); e.alpha = 1.f; }
    LAV_REQUIRE(!e.assign || (layout == 2 && e.out_mode == 2), "lav_gemm_bf16: assign is defined for weight gradients only (layout 2, out_mode 2)");
    if (e.alpha == 0.f) e.alpha = 1.f;
    if (splits < 1) splits = 1;
    LAV_REQUIRE(!e.rowsum_a || layout == 2, "lav_gemm_bf16: rowsum_a is only defined for layout 2 (TN)");
    const bool no_epilogue = !e.bias && !e.act && !e.preact && !e.gelu_in && e.dropout_p <= 0.f && !e.row_scale &&
                             !e.residual && !e.colsum && !e.rowsum_a && e.alpha == 1.f;
    LAV_REQUIRE(splits == 1 || e.out_mode == 2 || (e.out_mode == 0 && layout != 2 && no_epilogue && (N % 8) == 0),
                "lav_gemm_bf16: split-K needs out_mode=2 (fp32 accumulate), or a bf16 output without epilogue and N %% 8 == 0");
    LAV_REQUIRE(e.out_mode != 0 || (ldc % 8) == 0, "lav_gemm_bf16: bf16 output needs ldc %% 8 == 0");
    LAV_REQUIRE(e.hm_heads <= 0 || (e.out_mode == 0 && layout != 2 && splits == 1 && e.hm_head_dim > 0 && (e.hm_head_dim % 8) == 0 &&
                                    (N % (e.hm_heads * e.hm_head_dim)) == 0 && e.hm_rows >= M),
                "lav_gemm_bf16: head-major store needs a bf16 output, layout 0 / 1, no split-K, hm_head_dim %% 8 == 0, N %% (hm_heads * hm_head_dim) == 0 and hm_rows >= M");
    LAV_REQUIRE(e.out_mode == 0 || e.out_mode == 3 || (ldc % 4) == 0, "lav_gemm_bf16: fp32 output needs ldc %% 4 == 0");
    LAV_REQUIRE(e.out_mode != 3 || ((ldc % 8) == 0 && layout != 2 && splits == 1), "lav_gemm_bf16: fp16 output needs ldc %% 8 == 0, layout 0 / 1, no split-K");
    return LAV_OK;
}
// the two checks that depend on the route
static int gemm_plan_error(const GemmPlan& p, int layout, int N, int K, long ldc) {
    LAV_REQUIRE(p.err != GP_E_ROWMAP, "lav_gemm_bf16: a_rowmap needs layout 0, splits 1, N %% 256 == 0 and K %% 64 == 0 (got layout %d, N %d, K %d)", layout, N, K);
    LAV_REQUIRE(p.err != GP_E_ASSIGN_SPLITK, "lav_gemm_bf16: assign with split-K needs N %% 4 == 0 and ldc %% 4 == 0 (got N %d, ldc %ld)", N, ldc);
    return LAV_OK;
}

extern "C" int lav_gemm_bf16(void* stream, int layout, int M, int N, int K, const void* A, long lda, const void* B,
                             long ldb, void* C, long ldc, const lav_gemm_epilogue* epi, int splits) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    if (int rc = gemm_check_args(layout, M, N, K, true, A, lda, B, ldb, C, ldc, epi, g.e, splits)) return rc;
    const GemmPlan p = gemm_plan(layout, M, N, K, lda, ldb, ldc, g.e, splits, gemm_sw);
    if (int rc = gemm_plan_error(p, layout, N, K, ldc)) return rc;
    g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.M = M;
    g.drop_thresh = lav_drop_thresh(g.e.dropout_p);
    g.nt_preact = (gemm_sw.nt_stores & 1) | ((gemm_sw.nt_stores & 4) ? 2 : 0);
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < p.n_parts; ++i) {
        const GemmPart& q = p.part[i];
        g.A = (const bf16_t*)A + (long)q.k_off * lda; g.B = (const bf16_t*)B + (long)q.k_off * ldb;      // (k_off > 0: weight gradients, both operands [K, ld])
        g.N = q.N; g.K = q.K; g.nb_rows = q.nb_rows; g.k_per_split = q.k_per_split; g.splits = q.splits; g.group_n = q.group_n; g.dbg = q.dbg;
        g.owner = q.owner; g.assign = q.assign; g.ws_tiles = q.ws_tiles;          // (the kernels read GemmArgs.assign, never e.assign)
        g.ws = nullptr;
        if (q.ws_bytes) {
            g.ws = splitk_workspace(stream, q.ws_bytes);
            if (!g.ws) return LAV_E_WORKSPACE;               // message set by lav_ws_get
        }
        void* ga[] = {&g};
        gemm_launch(q.gemm, s, ga);
        if (q.reduce.kern >= 0) {                            // splitk_reduce_bf16_kernel takes the first nine of these, tn_reduce_kernel all ten
            int tiles_n = (q.N + BN - 1) / BN, rpt = q.rpt;
            void* ra[] = {&g.ws, &g.splits, &g.ws_tiles, &tiles_n, &rpt, &g.M, &g.N, &g.C, &g.ldc, &g.assign};
            gemm_launch(q.reduce, s, ra);
        }
        if (int rc = lav_check_launch("lav_gemm_bf16")) return rc;
    }
    return LAV_OK;
}

static void plan_report(const GemmLaunch& l, lav_gemm_launch_info* out, int max_out, int& n) {
    if (l.kern < 0) return;
    if (n < max_out) out[n] = {gemm_kernels[l.kern].name, l.tile_m, l.tile_n, l.grid, (unsigned)gemm_kernels[l.kern].threads};
    ++n;
}
// ws (optional) is raised to the LAV_WS_SPLITK bytes the call requests: its parts run one after the other on one stream and share the workspace
static int gemm_plan_query(int layout, int M, int N, int K, long lda, long ldb, long ldc, const lav_gemm_epilogue* epi, int splits,
                           lav_gemm_launch_info* out, int max_out, int& n, size_t* ws = nullptr) {
    lav_gemm_epilogue e;
    if (int rc = gemm_check_args(layout, M, N, K, false, nullptr, lda, nullptr, ldb, nullptr, ldc, epi, e, splits)) return rc;
    const GemmPlan p = gemm_plan(layout, M, N, K, lda, ldb, ldc, e, splits, gemm_sw);
    if (int rc = gemm_plan_error(p, layout, N, K, ldc)) return rc;
    for (int i = 0; i < p.n_parts; ++i) {
        plan_report(p.part[i].gemm, out, max_out, n); plan_report(p.part[i].reduce, out, max_out, n);
        if (ws && p.part[i].ws_bytes > *ws) *ws = p.part[i].ws_bytes;
    }
    return LAV_OK;
}
// the split factor of one call (splits <= 0: the library's own) and the workspace it takes; no device needed
extern "C" int lav_gemm_splits(int layout, int M, int N, int K, long lda, long ldb, long ldc, const lav_gemm_epilogue* epi, int splits, size_t* ws_bytes) {
    LAV_REQUIRE(M > 0 && N > 0 && K > 0, "lav_gemm_splits: empty problem M=%d N=%d K=%d", M, N, K);
    if (splits <= 0) splits = layout == 2 ? tn_splits(M, N, K, epi && epi->k_keep, gemm_sw) : nn_splits(M, N, K);
    int n = 0;
    if (ws_bytes) *ws_bytes = 0;
    if (ws_bytes)
        if (int rc = gemm_plan_query(layout, M, N, K, lda, ldb, ldc, epi, splits, nullptr, 0, n, ws_bytes)) return rc;
    return splits;
}
// probe hook: the launches lav_gemm_bf16 would make for this call, without making them (no device needed)
extern "C" int lav_gemm_plan(int layout, int M, int N, int K, long lda, long ldb, long ldc, const lav_gemm_epilogue* epi, int splits,
                             lav_gemm_launch_info* out, int max_out) {
    LAV_REQUIRE(out || max_out <= 0, "lav_gemm_plan: null output array");
    int n = 0;
    if (int rc = gemm_plan_query(layout, M, N, K, lda, ldb, ldc, epi, splits, out, max_out, n)) return rc;
    return n;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Grouped weight gradients: C_j (fp32, accumulated) += alpha_j * A_j^T B_j for up to four jobs in one launch of the ping-pong kernel.
// Every job must fit that kernel (>= 160 output rows (256 below 512 columns), N % 256 == 0, K % 32 == 0, the drop-path row rule);
// otherwise -- or with LAV_GEMM_TN_GROUP=0 -- the jobs run one by one through lav_gemm_bf16 with their own fallback split factors.
// ---------------------------------------------------------------------------------------------------------------------------------
static lav_gemm_epilogue tn_job_epilogue(const lav_gemm_tn_job& q) {          // the job as a lav_gemm_bf16 (layout 2) epilogue
    lav_gemm_epilogue e;
    memset(&e, 0, sizeof(e));
    e.alpha = q.alpha == 0.f ? 1.f : q.alpha; e.rows_per_group = 1; e.out_mode = 2; e.rowsum_a = q.rowsum_a; e.k_keep = q.k_keep;
    e.k_rows_per_group = q.k_keep ? q.k_rows_per_group : 1;
    e.assign = q.assign;
    return e;
}
static bool tn_group_fits(int n_jobs, const lav_gemm_tn_job* jobs, bool with_operands, const GemmSwitches& sw) {
    bool ok = sw.tn_group != 0;
    for (int j = 0; j < n_jobs && ok; ++j) {
        const lav_gemm_tn_job& q = jobs[j];
        ok = (!with_operands || (q.A && q.B && q.C && (((uintptr_t)q.A | (uintptr_t)q.B | (uintptr_t)q.C) & 15) == 0)) && q.N > 0 && q.K >= PP_BK &&
             (q.lda % 8) == 0 && (q.ldb % 8) == 0 && (q.ldc % 4) == 0 && tn_pp_fits(q.M, q.N, q.K, q.k_keep, q.k_rows_per_group, BKT, sw);
    }
    return ok;
}
// the grouped launch: per job its split (at least 256 contraction rows each), workspace slice and first block, and the blocks of the two launches
struct TnGroupPlan { int k_per_split[4], splits[4], ws_tiles[4], blk0[4], rblk0[4], blocks, rblocks; size_t ws_off[4], ws_bytes; };
static TnGroupPlan tn_group_plan(int n_jobs, const lav_gemm_tn_job* jobs, int splits) {
    TnGroupPlan p;
    memset(&p, 0, sizeof(p));
    for (int j = 0; j < n_jobs; ++j) {
        const lav_gemm_tn_job& q = jobs[j];
        int sp = splits;
        if (sp > q.K / TN_SPLIT_MIN_K) sp = q.K / TN_SPLIT_MIN_K > 0 ? q.K / TN_SPLIT_MIN_K : 1;
        p.k_per_split[j] = ((q.K + sp - 1) / sp + BKT - 1) / BKT * BKT;
        p.splits[j] = (q.K + p.k_per_split[j] - 1) / p.k_per_split[j];
        p.ws_tiles[j] = ((q.M + BIG_BM - 1) / BIG_BM) * ((q.N + BN - 1) / BN);
        p.blk0[j] = p.blocks;
        p.blocks += ((q.M + BIG_BM - 1) / BIG_BM) * (q.N / 256) * p.splits[j];
        if (p.splits[j] > 1) {
            p.ws_off[j] = p.ws_bytes;
            p.ws_bytes += (size_t)p.splits[j] * p.ws_tiles[j] * BIG_BM * BN * sizeof(float);
            p.rblk0[j] = p.rblocks;
            p.rblocks += (int)(((long)q.M * (q.N / 4) + 63) / 64);
        }
    }
    return p;
}

extern "C" int lav_gemm_tn_grouped(void* stream, int n_jobs, const lav_gemm_tn_job* jobs, int splits) {
    LAV_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= 4, "lav_gemm_tn_grouped: 1 ... 4 jobs (got %d)", n_jobs);
    if (splits < 1) splits = 1;
    if (!tn_group_fits(n_jobs, jobs, true, gemm_sw)) {
        for (int j = 0; j < n_jobs; ++j) {
            const lav_gemm_tn_job& q = jobs[j];
            const lav_gemm_epilogue e = tn_job_epilogue(q);
            if (int rc = lav_gemm_bf16(stream, 2, q.M, q.N, q.K, q.A, q.lda, q.B, q.ldb, q.C, q.ldc, &e, q.fallback_splits > 0 ? q.fallback_splits : 1)) return rc;
        }
        return LAV_OK;
    }
    const TnGroupPlan p = tn_group_plan(n_jobs, jobs, splits);
    float* ws = nullptr;
    if (p.ws_bytes) {
        ws = splitk_workspace(stream, p.ws_bytes);
        if (!ws) return LAV_E_WORKSPACE;                     // message set by lav_ws_get
    }
    GemmGroup G;
    TnReduceGroup R;
    memset(&G, 0, sizeof(G));
    memset(&R, 0, sizeof(R));
    G.n = n_jobs;
    G.walk = 3;                                              // launch-wide XCD runs, short-dimension-fastest tiles (profiles/r05_dw_walk.md; 0 = the round-4 walk)
    for (int j = 0; j < n_jobs; ++j) {
        const lav_gemm_tn_job& q = jobs[j];
        GemmArgs& g = G.g[j];
        g.A = (const bf16_t*)q.A; g.B = (const bf16_t*)q.B; g.C = q.C; g.lda = q.lda; g.ldb = q.ldb; g.ldc = q.ldc; g.M = q.M; g.N = q.N; g.K = q.K;
        g.e = tn_job_epilogue(q);
        g.e.assign = 0;                                      // (the kernels read GemmArgs.assign)
        g.assign = q.assign != 0;
        g.k_per_split = p.k_per_split[j];
        g.splits = p.splits[j];
        G.blk0[j] = p.blk0[j];
        if (g.splits == 1) { g.owner = 1; continue; }
        g.ws = (float*)((char*)ws + p.ws_off[j]); g.ws_tiles = p.ws_tiles[j];
        TnReduceJob& r = R.j[R.n++];
        r.ws = g.ws; r.C = (float*)g.C; r.ldc = g.ldc; r.splits = g.splits; r.tiles = p.ws_tiles[j]; r.tiles_n = (g.N + BN - 1) / BN; r.rpt = BIG_BM; r.M = g.M; r.N = g.N;
        r.blk0 = p.rblk0[j]; r.assign = g.assign;
    }
    hipStream_t s = (hipStream_t)stream;
    void* ga[] = {&G};
    gemm_launch({GK_PP_GROUP, (unsigned)p.blocks, 256, 256}, s, ga);
    void* ra[] = {&R};
    if (R.n) gemm_launch({GK_TN_REDUCE_GROUP, (unsigned)p.rblocks, 256, BN}, s, ra);
    return lav_check_launch("lav_gemm_tn_grouped");
}

// probe hook: the launches lav_gemm_tn_grouped would make (one grouped launch, or the job-by-job fallback), without making them
extern "C" int lav_gemm_tn_grouped_plan(int n_jobs, const lav_gemm_tn_job* jobs, int splits, lav_gemm_launch_info* out, int max_out) {
    LAV_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= 4, "lav_gemm_tn_grouped: 1 ... 4 jobs (got %d)", n_jobs);
    LAV_REQUIRE(out || max_out <= 0, "lav_gemm_tn_grouped_plan: null output array");
    if (splits < 1) splits = 1;
    int n = 0;
    if (!tn_group_fits(n_jobs, jobs, false, gemm_sw)) {
        for (int j = 0; j < n_jobs; ++j) {
            const lav_gemm_tn_job& q = jobs[j];
            const lav_gemm_epilogue e = tn_job_epilogue(q);
            if (int rc = gemm_plan_query(2, q.M, q.N, q.K, q.lda, q.ldb, q.ldc, &e, q.fallback_splits > 0 ? q.fallback_splits : 1, out, max_out, n)) return rc;
        }
        return n;
    }
    const TnGroupPlan p = tn_group_plan(n_jobs, jobs, splits);
    plan_report({GK_PP_GROUP, (unsigned)p.blocks, 256, 256}, out, max_out, n);
    if (p.rblocks) plan_report({GK_TN_REDUCE_GROUP, (unsigned)p.rblocks, 256, BN}, out, max_out, n);
    return n;
}

// the group factor over jobs that fit the grouped launch (tn_group_fits): tn_group_blocks workgroups, at least TN_SPLIT_MIN_K contraction rows each
static int tn_group_splits(int n_jobs, const lav_gemm_tn_job* jobs, const GemmSwitches& sw) {
    int tiles = 0, K = jobs[0].K;
    for (int j = 0; j < n_jobs; ++j) {
        tiles += ((jobs[j].M + BIG_BM - 1) / BIG_BM) * (jobs[j].N / 256);
        if (jobs[j].K < K) K = jobs[j].K;
    }
    const int blocks = tiles >= 96 ? sw.tn_group_blocks_wide : sw.tn_group_blocks;
    return clamp_splits((int)nearbyint((double)blocks / tiles), K / TN_SPLIT_MIN_K);          // (halves round to even, as they always did)
}
// the split factors of a stage's weight gradients and the workspace they take; no device needed
extern "C" int lav_gemm_tn_splits(int n_jobs, lav_gemm_tn_job* jobs, int splits, size_t* ws_bytes) {
    LAV_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= 4, "lav_gemm_tn_splits: 1 ... 4 jobs (got %d)", n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        lav_gemm_tn_job& q = jobs[j];
        LAV_REQUIRE(q.M > 0 && q.N > 0 && q.K > 0, "lav_gemm_tn_splits: empty problem M=%d N=%d K=%d", q.M, q.N, q.K);
        if (q.fallback_splits <= 0) q.fallback_splits = tn_splits(q.M, q.N, q.K, q.k_keep != nullptr, gemm_sw);
    }
    const int group = !tn_group_fits(n_jobs, jobs, false, gemm_sw) ? 0 : splits > 0 ? splits : tn_group_splits(n_jobs, jobs, gemm_sw);
    if (ws_bytes) *ws_bytes = group ? tn_group_plan(n_jobs, jobs, group).ws_bytes : 0;
    for (int j = 0, n = 0; ws_bytes && j < n_jobs; ++j) {
        const lav_gemm_tn_job& q = jobs[j];
        const lav_gemm_epilogue e = tn_job_epilogue(q);
        if (int rc = gemm_plan_query(2, q.M, q.N, q.K, q.lda, q.ldb, q.ldc, &e, q.fallback_splits, nullptr, 0, n, ws_bytes)) return rc;
    }
    return group;
}
