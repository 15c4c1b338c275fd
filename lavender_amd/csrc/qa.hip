// Video question answering read-out (eval only): what Agent_QAOE_MLM / Agent_QAMC_MLM take from the (n, V) logit rows of the labelled
// [MASK] positions (main_qaoe_mlm_lsmdc_fib.py:115-126, main_qamc_mlm.py:159-166), in ONE pass over each row:
//   pred     arg-max column
//   rank     number of columns that sort before the label's column (a top-k hit is 0 <= rank < k)
//   choice   arg-max over the candidate tokens of x_cand[c] / sum_c x_cand[c] (raw logits, as the reference divides them)
// Order of the columns: value descending, a NaN above every number (torch.topk / torch.argmax), the lower index first among equals.  Every
// value becomes a 32-bit key that sorts like it and (key, ~index) one 64-bit word, so "the best column" is an integer max and "sorts before
// the label" an integer compare: counts and the max do not depend on how a row is cut into lanes, waves or workgroups, and the results are
// bit-identical for every split count.  With splits > 1 each row is cut into `splits` column ranges, one workgroup each, and a second small
// launch merges the per-range partials from the caller's workspace: no atomics, no last-block counter.
#include "common.h"
#include "../../include/lavender_hip.h"

#define AQ_THREADS 256
#define AQ_WAVES (AQ_THREADS / 64)
typedef unsigned long long aq_u64;

struct aq_cand { int32_t id[LAV_ANSWER_MAX_CAND]; };

// sorts like the value: -inf < ... < -0 = +0 < ... < +inf < NaN
__device__ __forceinline__ uint32_t aq_key(float x) {
    if (x != x) return 0xFFFFFFFFu;
    uint32_t u = __float_as_uint(x);
    if ((u << 1) == 0u) u = 0u;                            // -0 and +0 are one value
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// larger word = earlier in the order; every real column gives a word > 0 (the key of -inf is 0x007fffff), so 0 is the "no column" identity
__device__ __forceinline__ aq_u64 aq_word(float x, int c) { return ((aq_u64)aq_key(x) << 32) | (uint32_t)(~(uint32_t)c); }

template <bool F32>
__device__ __forceinline__ float aq_load(const char* row, int c) {
    return F32 ? ((const float*)row)[c] : bf2f(((const bf16_t*)row)[c]);
}

__device__ __forceinline__ aq_u64 aq_shfl_xor(aq_u64 v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    return ((aq_u64)hi << 32) | lo;
}

// main_qamc_mlm.py:159-166 on one row: fp32 sum in candidate order, fp32 quotients, first index wins, NaN above every number
template <bool F32>
__device__ int aq_choice(const char* row, const aq_cand& cand, int n_cand) {
    if (n_cand <= 0) return -1;
    float sum = 0.f;
    for (int c = 0; c < n_cand; ++c) sum += aq_load<F32>(row, cand.id[c]);
    aq_u64 best = 0;
    for (int c = 0; c < n_cand; ++c) {
        const aq_u64 w = aq_word(aq_load<F32>(row, cand.id[c]) / sum, c);
        best = w > best ? w : best;
    }
    return (int)(~(uint32_t)best);
}

template <bool F32>
__global__ __launch_bounds__(AQ_THREADS) void answer_readout_kernel(int V, const char* __restrict__ x, long ld, const int32_t* __restrict__ labels,
                                                                   aq_cand cand, int n_cand, int splits, aq_u64* __restrict__ part_best,
                                                                   int32_t* __restrict__ part_cnt, int32_t* __restrict__ pred,
                                                                   int32_t* __restrict__ rank, int32_t* __restrict__ choice) {
    constexpr int ES = F32 ? 4 : 2, VE = 16 / ES;
    __shared__ aq_u64 sbest[AQ_WAVES];
    __shared__ int scnt[AQ_WAVES];
    const int r = blockIdx.x / splits, s = blockIdx.x % splits, tid = threadIdx.x;
    const char* row = x + (long)r * ld * ES;
    int t = labels[r];
    if (t < 0 || t >= V) t = -1;                           // the entry rejects other labels where it can see them; never read outside the row
    const aq_u64 wt = t >= 0 ? aq_word(aq_load<F32>(row, t), t) : ~(aq_u64)0;   // no column sorts before the all-ones word
    // this workgroup's columns [c0, c1): scalar head up to the first 16-byte boundary, 16-byte body, scalar tail
    const int per = (V + splits - 1) / splits;
    const int c0 = min(V, s * per), c1 = min(V, c0 + per);
    const int head = (int)(((16u - (uint32_t)((uintptr_t)(row + (long)c0 * ES) & 15u)) & 15u) / ES);
    const int v0 = min(c1, c0 + head);
    const int nvec = (c1 - v0) / VE, v1 = v0 + nvec * VE;
    aq_u64 best = 0;
    int cnt = 0;
    for (int c = c0 + tid; c < v0; c += AQ_THREADS) {
        const aq_u64 w = aq_word(aq_load<F32>(row, c), c);
        best = w > best ? w : best;
        cnt += w > wt ? 1 : 0;
    }
    const uint4* vp = (const uint4*)(row + (long)v0 * ES);
    for (int i = tid; i < nvec; i += AQ_THREADS) {
        const uint4 v = vp[i];
        float f[8];
        if (F32) { f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w); }
        else unpack8(v, f);
#pragma unroll
        for (int k = 0; k < VE; ++k) {
            const aq_u64 w = aq_word(f[k], v0 + i * VE + k);
            best = w > best ? w : best;
            cnt += w > wt ? 1 : 0;
        }
    }
    for (int c = v1 + tid; c < c1; c += AQ_THREADS) {
        const aq_u64 w = aq_word(aq_load<F32>(row, c), c);
        best = w > best ? w : best;
        cnt += w > wt ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const aq_u64 ob = aq_shfl_xor(best, o);
        best = ob > best ? ob : best;
        cnt += __shfl_xor(cnt, o, 64);
    }
    if ((tid & 63) == 0) { sbest[tid >> 6] = best; scnt[tid >> 6] = cnt; }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < AQ_WAVES; ++w) {
        best = sbest[w] > best ? sbest[w] : best;
        cnt += scnt[w];
    }
    if (splits > 1) {
        part_best[blockIdx.x] = best;
        part_cnt[blockIdx.x] = cnt;
        return;
    }
    pred[r] = (int)(~(uint32_t)best);
    rank[r] = t >= 0 ? cnt : -1;
    choice[r] = aq_choice<F32>(row, cand, n_cand);
}

// splits > 1: one thread per row folds that row's partials in split order (integer max and sum: any order gives the same bits)
template <bool F32>
__global__ __launch_bounds__(64) void answer_merge_kernel(int n, int V, const char* __restrict__ x, long ld, const int32_t* __restrict__ labels, aq_cand cand,
                                                         int n_cand, int splits, const aq_u64* __restrict__ part_best,
                                                         const int32_t* __restrict__ part_cnt, int32_t* __restrict__ pred, int32_t* __restrict__ rank,
                                                         int32_t* __restrict__ choice) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n) return;
    aq_u64 best = 0;
    int cnt = 0;
    for (int s = 0; s < splits; ++s) {
        const aq_u64 b = part_best[(long)r * splits + s];
        best = b > best ? b : best;
        cnt += part_cnt[(long)r * splits + s];
    }
    const int t = labels[r];
    pred[r] = (int)(~(uint32_t)best);
    rank[r] = (t >= 0 && t < V) ? cnt : -1;
    choice[r] = aq_choice<F32>(x + (long)r * ld * (F32 ? 4 : 2), cand, n_cand);
}

extern "C" size_t lav_answer_readout_workspace_bytes(int n, int splits) {
    return (n <= 0 || splits <= 1) ? 0 : (size_t)n * (size_t)splits * (sizeof(aq_u64) + sizeof(int32_t));
}

extern "C" int lav_answer_readout(void* stream, int n, int V, const void* logits, long ld, int dtype, const int32_t* labels,
                                  const int32_t* labels_host, const int32_t* cand_host, int n_cand, int splits, void* workspace,
                                  size_t workspace_bytes, int32_t* pred, int32_t* rank, int32_t* choice) {
    LAV_REQUIRE(n > 0 && V > 0 && ld >= V && (long)n * splits <= 0x7fffffffL, "lav_answer_readout: n=%d V=%d ld=%ld (ld >= V)", n, V, ld);
    LAV_REQUIRE(dtype == 0 || dtype == 1, "lav_answer_readout: dtype=%d (0 bf16, 1 fp32)", dtype);
    LAV_REQUIRE(splits >= 1 && splits <= LAV_ANSWER_MAX_SPLITS, "lav_answer_readout: splits=%d (1..%d)", splits, LAV_ANSWER_MAX_SPLITS);
    LAV_REQUIRE(n_cand >= 0 && n_cand <= LAV_ANSWER_MAX_CAND && (n_cand == 0 || cand_host), "lav_answer_readout: n_cand=%d (0..%d, with a host array)",
                n_cand, LAV_ANSWER_MAX_CAND);
    LAV_REQUIRE(logits && labels && pred && rank && choice, "lav_answer_readout: null pointer");
    LAV_REQUIRE(((uintptr_t)logits % (dtype == 1 ? 4 : 2)) == 0, "lav_answer_readout: logits are not aligned to their element size");
    aq_cand cand;
    memset(&cand, 0, sizeof(cand));
    for (int c = 0; c < n_cand; ++c) {
        LAV_REQUIRE(cand_host[c] >= 0 && cand_host[c] < V, "lav_answer_readout: candidate %d = token %d outside [0, %d)", c, cand_host[c], V);
        cand.id[c] = cand_host[c];
    }
    if (labels_host)
        for (int r = 0; r < n; ++r)
            LAV_REQUIRE(labels_host[r] >= -1 && labels_host[r] < V, "lav_answer_readout: label %d of row %d outside [0, %d) and not -1", labels_host[r], r, V);
    aq_u64* pb = nullptr;
    int32_t* pc = nullptr;
    if (splits > 1) {
        const size_t need = lav_answer_readout_workspace_bytes(n, splits);
        if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7) != 0) {
            lav_set_error("lav_answer_readout: %d rows in %d splits need an 8-byte aligned workspace of %zu bytes (lav_answer_readout_workspace_bytes), got %zu",
                          n, splits, need, workspace ? workspace_bytes : (size_t)0);
            return LAV_E_WORKSPACE;
        }
        pb = (aq_u64*)workspace;
        pc = (int32_t*)(pb + (size_t)n * splits);
    }
    const dim3 grid((unsigned)n * splits), mgrid((n + 63) / 64);
    const char* x = (const char*)logits;
    if (dtype == 1) {
        hipLaunchKernelGGL(answer_readout_kernel<true>, grid, dim3(AQ_THREADS), 0, (hipStream_t)stream, V, x, ld, labels, cand, n_cand, splits, pb, pc,
                           pred, rank, choice);
        if (splits > 1)
            hipLaunchKernelGGL(answer_merge_kernel<true>, mgrid, dim3(64), 0, (hipStream_t)stream, n, V, x, ld, labels, cand, n_cand, splits, pb, pc,
                               pred, rank, choice);
    } else {
        hipLaunchKernelGGL(answer_readout_kernel<false>, grid, dim3(AQ_THREADS), 0, (hipStream_t)stream, V, x, ld, labels, cand, n_cand, splits, pb, pc,
                           pred, rank, choice);
        if (splits > 1)
            hipLaunchKernelGGL(answer_merge_kernel<false>, mgrid, dim3(64), 0, (hipStream_t)stream, n, V, x, ld, labels, cand, n_cand, splits, pb, pc,
                               pred, rank, choice);
    }
    return lav_check_launch("lav_answer_readout");
}

// ---- in-batch matching read-out (retrieval / lsmdc-mc evaluation): main_retrieval_mlm.py:107-118, main_retmc_mlm.py:129-140 ----------------------
// One wave per group of O candidates, lanes stride over o; the arg-max is the integer max of the (key, ~o) word above, so it does not depend on O
// or on which lane met which candidate.  A candidate whose row lies outside the block reads nothing and takes key 0, below the key of -inf.
#define MR_THREADS 256
#define MR_WAVES (MR_THREADS / 64)
#define MR_MAX_BLOCKS 2048

template <bool F32>
__global__ __launch_bounds__(MR_THREADS) void match_readout_kernel(int G, int O, const char* __restrict__ x, long ld, const int32_t* __restrict__ row,
                                                                  long n_rows, int true_col, int false_col, const int32_t* __restrict__ gt,
                                                                  float* __restrict__ score, int32_t* __restrict__ choice, int32_t* __restrict__ hit) {
    constexpr int ES = F32 ? 4 : 2;
    const int lane = threadIdx.x & 63;
    for (long g = (long)blockIdx.x * MR_WAVES + (threadIdx.x >> 6); g < G; g += (long)gridDim.x * MR_WAVES) {   // uniform within a wave
        aq_u64 best = 0;
        for (int o = lane; o < O; o += 64) {
            const long k = g * O + o;
            const long r = row ? (long)row[k] : k;
            float s = __uint_as_float(0x7fc00000u);
            aq_u64 w = (uint32_t)(~(uint32_t)o);                 // key 0: the "NaN-last" class
            if (r >= 0 && r < n_rows) {
                const char* p = x + r * ld * ES;
                const float t = aq_load<F32>(p, true_col), f = aq_load<F32>(p, false_col);
                s = t / (t + f);
                if (s != s) s = __uint_as_float(0x7fc00000u);   // one NaN pattern in `score`, whatever the division made
                w = aq_word(s, o);
            }
            if (score) score[k] = s;
            best = w > best ? w : best;
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const aq_u64 ob = aq_shfl_xor(best, m);
            best = ob > best ? ob : best;
        }
        if (lane == 0) {
            const int c = (int)(~(uint32_t)best);
            choice[g] = c;
            if (hit) hit[g] = (c == gt[g]) ? 1 : 0;             // c lies in [0, O): a gt outside it never hits
        }
    }
}

extern "C" int lav_match_readout(void* stream, int G, int O, const void* logits, long ld, int dtype, const int32_t* row, long n_rows, int true_col,
                                 int false_col, const int32_t* gt, float* score, int32_t* choice, int32_t* hit) {
    LAV_REQUIRE(G >= 1 && O >= 1, "lav_match_readout: G=%d O=%d (both >= 1)", G, O);
    LAV_REQUIRE(dtype == 0 || dtype == 1, "lav_match_readout: dtype=%d (0 bf16, 1 fp32)", dtype);
    LAV_REQUIRE(ld >= 1 && true_col >= 0 && true_col < ld && false_col >= 0 && false_col < ld,
                "lav_match_readout: columns %d / %d outside [0, ld = %ld)", true_col, false_col, ld);
    LAV_REQUIRE(n_rows >= 0 && (row || n_rows >= (long)G * O), "lav_match_readout: %ld rows for %d x %d candidates and no row map", n_rows, G, O);
    LAV_REQUIRE(logits && choice && (!hit || gt), "lav_match_readout: null pointer (logits, choice, or hit without gt)");
    LAV_REQUIRE(((uintptr_t)logits % (dtype == 1 ? 4 : 2)) == 0, "lav_match_readout: logits are not aligned to their element size");
    const long blocks = ((long)G + MR_WAVES - 1) / MR_WAVES;
    const dim3 grid((unsigned)(blocks < MR_MAX_BLOCKS ? blocks : MR_MAX_BLOCKS));
    if (dtype == 1)
        hipLaunchKernelGGL(match_readout_kernel<true>, grid, dim3(MR_THREADS), 0, (hipStream_t)stream, G, O, (const char*)logits, ld, row, n_rows,
                           true_col, false_col, gt, score, choice, hit);
    else
        hipLaunchKernelGGL(match_readout_kernel<false>, grid, dim3(MR_THREADS), 0, (hipStream_t)stream, G, O, (const char*)logits, ld, row, n_rows,
                           true_col, false_col, gt, score, choice, hit);
    return lav_check_launch("lav_match_readout");
}
