// Shared pieces of the attention kernels (forward, dQ pass, dK/dV pass).
//
// MFMA shape: v_mfma_f32_32x32x16_bf16.  Operand lane maps (lane l, hi = l>>5, j = l&31):
//   A[i=j][k=8hi..8hi+7], B[k=8hi..8hi+7][j], C/D[row=(r&3)+8(r>>2)+4hi][col=j], r in [0,16).
// All three kernels compute score tiles "transposed" so that the softmax row (one query, or one key in
// the dK/dV pass) is lane-local: a lane owns one column j and 16 rows of each 32x32 tile.
#pragma once
#include "common.h"
#include "../../include/lavender_hip.h"

struct AttnArgs {
    lav_attn_desc d;
    const bf16_t* qkv; const bf16_t* out; const bf16_t* dout;
    bf16_t* o_w; float* lse; bf16_t* dqkv; float* dbias;
    int N;            // tokens per problem (window volume or sequence length)
    int Npad;         // lse row stride
    int nqt;          // ceil(N/32)
    int nWd, nWh, nWw;
    int C;            // heads*head_dim
    int tbl_rows, tbl_const, cstride_d, cstride_h;   // bias-table geometry
    int R;            // 32-row tiles per wave
    uint32_t thresh;
    uint32_t thresh16; // sequence mode: dropout threshold on the 16-bit hash fields (one 64-bit hash per group of four keys: lav_hash64)
    int NH;           // ceil(N/4): key groups per query row
    int nWs, tps;     // windows per sample, tokens per sample (fast window path)
};

int attn_setup(const lav_attn_desc* d, AttnArgs& a, int& problems);

// ---- route plan (attention.hip: attn_plan) -------------------------------------------------------------------------------------
// LDS geometry of the specialised kernels: the plan sizes their launches with it, the kernels lay their LDS out with it.
#define WL_ROWS 768                                        // large windows (attention_winl.hip): rows of an operand image
#define WL_IMG (WL_ROWS * 64)
#define WLB_BUF (16384 * 2 + 8192 * 2 + 2048 + 384 * 4 * 2)
#define WLB_DLD 257
#define WLB_MAIN (2 * WLB_BUF > 128 * WLB_DLD * 4 ? 2 * WLB_BUF : 128 * WLB_DLD * 4)
#define SEQ3_ROWS 288                                      // one-image sequences (attention_seq.hip): LDS image rows
#define SEQ3_IMG (SEQ3_ROWS * 128)
#define SEQL_ROWS 768                                      // chunked sequences
#define SEQL_CH 256                                        // rows per chunk
#define SEQL_IMG (SEQL_CH * 128)
#define SEQL_BUF (2 * SEQL_IMG)
#define WIN_KL 256                                         // generic kernels (attention.hip): keys / queries staged per pass
#define SEQ_KL_FWD 288   // forward: K/V of a whole fusion sequence (L <= 288) staged once, two blocks per CU
#define SEQ_KL 128       // backward dQ pass: 128-key chunks -> 48 KB of LDS, the register file (not LDS) sets the occupancy
#define SEQ_QL 128       // backward dK/dV pass: 128-query chunks (4 staged copies = 64 KB): two blocks per CU instead of one

struct WlTab { int lo, n, mc; };     // large windows: first reachable bias-table row, reachable rows, code of the last window slot

enum AttnRoute { AR_WIN_PERSISTENT, AR_WIN_LARGE, AR_SEQ_ONE, AR_SEQ_CHUNKED, AR_GEN_WINDOW, AR_GEN_SEQ, AR_COUNT };
enum AttnPass { AP_FWD, AP_BWD, AP_BWD_BIAS, AP_BIAS, AP_COUNT };   // forward; dQ / dK / dV; the same + bias-table gradient; that gradient alone
enum AttnKernelId {                                                 // family by family: a launch goes to the file that holds its kernel
    AK_WIN_FWD3, AK_WIN_BWD1, AK_WIN_DBIAS3, AK_WINL_FWD, AK_WINL_DQ, AK_WINL_DKV, AK_WINL_DBIAS,
    AK_SEQ_FWD3, AK_SEQ_DQ3, AK_SEQ_DKV3, AK_SEQL_FWD, AK_SEQL_DQ, AK_SEQL_DKV, AK_GEN_FWD, AK_GEN_DQ, AK_GEN_DKV, AK_COUNT
};
// One launch.  split = the kernel's own partition scalar: bsplit (batch slices per (head, window position): win_*), QS (query parts per problem:
// winl_fwd / dq / dkv), WS (window slices: winl_dbias), parts (8-tile parts per problem: seql_*), R (32-row tiles per wave: generic); 0 = none.
struct AttnLaunch { int kern; unsigned grid_x, grid_y, block; size_t lds; int split; };
struct AttnPlan {
    AttnRoute route;
    int NT;                // 32-row tiles of a problem (the persistent kernels' template argument)
    WlTab tab;             // AR_WIN_LARGE
    bool bias_split;       // the bias-table gradient can run as its own launch (AP_BIAS is not empty)
    bool delta_negated;    // the backward leaves -delta behind the lse (win_bwd1 writes it, win_dbias3 reads it); every other route +delta
    int n[AP_COUNT];       // launches of each pass, in order (AP_BIAS: 0 = lav_attention_bwd has to produce the bias-table gradient)
    AttnLaunch launch[AP_COUNT][3];
};
// the process switches: LAV_WINL / LAV_SEQL (0 = generic kernels for large windows / long sequences) and lav_winl_select's query parts
struct AttnSwitches { bool winl, seql; int winl_parts; };
AttnPlan attn_plan(const AttnArgs& a, int problems, const AttnSwitches& sw);

// the families' launch functions: one planned launch of a kernel they hold (delta: the scratch behind the lse)
void win_launch(hipStream_t s, const AttnArgs& a, const AttnPlan& p, const AttnLaunch& l, float* delta);      // attention_win.hip
void winl_launch(hipStream_t s, const AttnArgs& a, const AttnPlan& p, const AttnLaunch& l, float* delta);     // attention_winl.hip
void seq_launch(hipStream_t s, const AttnArgs& a, const AttnPlan& p, const AttnLaunch& l, float* delta);      // attention_seq.hip

// raises the kernel's dynamic-LDS limit to the launch's bytes and launches it; the arguments convert to the kernel's parameter types
template <typename T> struct AttnParam { typedef T type; };
template <typename... P>
static void attn_launch(void (*kern)(P...), const AttnLaunch& l, hipStream_t s, typename AttnParam<P>::type... args) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds);
    (void)hipGetLastError();
    void* av[] = {(void*)&args...};
    (void)hipLaunchKernel((const void*)kern, dim3(l.grid_x, l.grid_y), dim3(l.block), av, l.lds, s);
}

__device__ __forceinline__ int tile_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// Cross-half exchange of a wave64 (lane j <-> lane j + 32) without the LDS round trip of ds_bpermute_b32: v_permlane32_swap_b32
// (gfx950) returns the lower half's values in every lane (lo) and the upper half's values in every lane (hi).
__device__ __forceinline__ void half_swap(float v, float& lo, float& hi) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    lo = __uint_as_float(r[0]); hi = __uint_as_float(r[1]);
}
__device__ __forceinline__ float xhalf_max(float v) { float lo, hi; half_swap(v, lo, hi); return fmaxf(lo, hi); }
__device__ __forceinline__ float xhalf_add(float v) { float lo, hi; half_swap(v, lo, hi); return lo + hi; }
__device__ __forceinline__ float lower_half(float v) { float lo, hi; half_swap(v, lo, hi); return lo; }

// two exponent arguments with ONE v_pk_fma_f32 (packed fp32: both halves of the 64-bit register pair in one issue slot)
typedef float lav_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ lav_f2 fma2(float a0, float a1, float b, float c0, float c1) {
    const lav_f2 a = {a0, a1}, bb = {b, b}, c = {c0, c1};
    return __builtin_elementwise_fma(a, bb, c);
}
__device__ __forceinline__ lav_f2 mul2(float a0, float a1, float b0, float b1) {
    const lav_f2 a = {a0, a1}, b = {b0, b1};
    return a * b;
}

struct TokInfo { int row; int code; int region; };

// window w, in-window index i  ->  global token row (un-rolled tensor), bias code, shift region
__device__ __forceinline__ TokInfo win_token(const AttnArgs& a, int win, int i) {
    const lav_attn_desc& d = a.d;
    int wwi = win % a.nWw, t = win / a.nWw;
    int whi = t % a.nWh; t /= a.nWh;
    int wdi = t % a.nWd, b = t / a.nWd;
    int wi = i % d.ww, t2 = i / d.ww;
    int hi = t2 % d.wh, di = t2 / d.wh;
    int pd = wdi * d.wd + di, ph = whi * d.wh + hi, pw = wwi * d.ww + wi;     // coordinates in the rolled tensor
    int sd_ = pd + d.sd, sh_ = ph + d.sh, sw_ = pw + d.sw;                    // roll(-shift): rolled[p] = x[(p+s) % n]
    if (sd_ >= d.D) sd_ -= d.D;
    if (sh_ >= d.H) sh_ -= d.H;
    if (sw_ >= d.W) sw_ -= d.W;
    TokInfo o;
    o.row = ((b * d.D + sd_) * d.H + sh_) * d.W + sw_;
    // relative_position_index[:N, :N] of the CONFIGURED window (video_swin.py:153): index i is decoded with the configured
    // (h, w) extents -- identical to (di, hi, wi) unless the spatial window is clamped
    o.code = (i / (d.cfg_wh * d.cfg_ww)) * a.cstride_d + ((i / d.cfg_ww) % d.cfg_wh) * a.cstride_h + (i % d.cfg_ww);
    int rd = d.sd ? (pd >= d.D - d.wd) + (pd >= d.D - d.sd) : 0;
    int rh = d.sh ? (ph >= d.H - d.wh) + (ph >= d.H - d.sh) : 0;
    int rw = d.sw ? (pw >= d.W - d.ww) + (pw >= d.W - d.sw) : 0;
    o.region = rd * 9 + rh * 3 + rw;
    return o;
}

// K-type LDS tile: rows of HD bf16 (d contiguous), 16-byte slots XOR-swizzled so that the 32x32 A-operand
// read (32 rows x one slot) is bank-conflict-free.
// slot XOR of a 128-byte-row (head_dim 64) image: a permutation of (row >> 1) & 7 -- the eight row pairs of a 16-row ds_read_b128 group
// still land on eight distinct bank groups -- chosen so that rows r and r + 2 (same bank half) differ by 4, not 1: the two adjacent
// slots a ds_read_b64_tr_b16 group takes from rows r .. r + 3 then never coincide.
__device__ __forceinline__ int swz64(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }

template <int HD>
__device__ __forceinline__ int krow_off(int row, int slot) {
    if (HD == 32) return row * 64 + ((slot ^ ((row >> 2) & 3)) << 4);
    // LDS has 64 banks (256 B per cycle): two consecutive 128-byte rows sweep the banks once, so the slot XOR advances every SECOND row --
    // 16 consecutive rows then hit 16 distinct 16-byte bank groups.  (XOR by row & 7 was tried in round 3: SQ_LDS_BANK_CONFLICT doubled.)
    return row * 128 + ((slot ^ swz64(row)) << 4);
}

__device__ __forceinline__ bf16x8 as_bf16x8(uint4 v) {
    union { uint4 u; bf16x8 b; } x; x.u = v; return x.b;
}
__device__ __forceinline__ bf16x8 pack_frag(const float* p) {
    union { uint4 u; bf16x8 b; } x; x.u = pack8(p); return x.b;
}

typedef __attribute__((address_space(3))) s16x4 lds_s16x4_t;

template <int HD>
__device__ __forceinline__ int vrow_off(int row, int slot) {
    if (HD == 32) return row * 64 + (slot << 4);
    return row * 128 + ((slot ^ (((row >> 1) & 1) << 2)) << 4);
}

// A-operand (32 rows of the transposed tile = 32 d-values, 16 keys) from a row-major [key][HD] LDS tile.
// lane (j = l&31 -> d = d0 + j, hi): keys key0 + {4hi..4hi+3} and key0 + 8 + {4hi..4hi+3}
template <int HD>
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int key0, int d0, int lane) {
    const int i = lane & 15, dhalf = (lane >> 4) & 1, hi = lane >> 5;
    const int r = i >> 2, c = i & 3;
    const int dcol = d0 + 16 * dhalf + 4 * c;                 // first of 4 d-columns this lane's address covers
    const int slot = dcol >> 3, sub = (dcol & 7) * 2;
    const int row0 = key0 + 4 * hi + r;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(tile + vrow_off<HD>(row0, slot) + sub));
    s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(tile + vrow_off<HD>(row0 + 8, slot) + sub));
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = lo; u.s.b = hi4;
    return u.v;
}

