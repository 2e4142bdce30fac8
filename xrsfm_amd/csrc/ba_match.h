// Batched SIFT descriptor matching on the int8 matrix cores: SiftMatchGPU::GetSiftMatch for every candidate pair of FeatureMatching
// (reference src/feature/feature_processing.cc:118-154, 240-255; 3rdparty/SiftGPU/ProgramCU.cu:1491-1884).  The rule is in
// ba_match_rule.h; this file spreads it over three kernels.
//
// The i8 matrix instruction is signed and the descriptors are not: a' = a ^ 0x80 read as int8 is a - 128, so
//   dot(i, j) = sum a'b' + 128 (sum a'_i + sum b'_j) + 2^21,   |sum a'b'| <= 2^21: everything stays in int32.
// k_match_prep flips the bytes of every descriptor that takes part, in place, and writes 128 * sum a' per descriptor.
//
// k_match_dots: one 256-thread workgroup per work item (pair, strip of kMatchStrip = 128 rows of A).  Wave w owns rows 32 w .. 32 w
// + 31 of the strip as two 16-row tiles whose fragments (two K-steps of 64 bytes) stay in registers for the whole walk.  B passes
// through LDS in blocks of kMatchCols = 64 columns (rows padded to 144 bytes against bank conflicts), shared by the four waves;
// the next block's global loads are issued before the current block's arithmetic.  v_mfma_i32_16x16x64_i8 with the A rows as its
// A operand leaves, in lane l and register r of a tile, the score of row 4 (l >> 4) + r and column l & 15.  Both operands are 16
// consecutive descriptor bytes per lane and K-step, so the order of k inside the instruction is the same on both sides and drops
// out of the sum.  Every lane keeps the running triples of its eight rows over the columns it sees (ascending) and merges them
// across the 16 lanes of a row once at the end.  Per column tile it keeps the triple of its column over its eight rows
// (ascending), merges across the four lane groups, and the four waves' triples go through LDS and are merged in wave order: the
// strip's partial [strip][n_b] (the role of the reference's texCRT).  Padding rows and columns get an offset term of -2^29, so
// their scores are negative: they can neither become a best nor raise a next.
//
// k_match_select: one workgroup per pair.  It merges the column partials over the strips in strip order, applies the test through
// the table to columns and rows, and writes the matches compacted in ascending i (ballot and prefix sums in a fixed order) at the
// pair's upper-bound offset, with the three counts.
//
// Integer arithmetic only, but for the one float multiply and two compares of the test.  No atomics; nothing waits for another
// workgroup; every loop is bounded by n_a, n_b <= 16384; a pair's outputs depend on nothing but the pair.
#pragma once
#include "ba_match_rule.h"

namespace xba {

constexpr int kMatchThreads = 256;
constexpr int kMatchStrip = 128;               // rows of A per workgroup: 32 per wave, two 16-row tiles
constexpr int kMatchCols = 64;                 // columns of B per LDS block: four 16-column tiles
constexpr int kMatchLdsRow = 144;              // bytes of a staged descriptor (128 + 16 of padding)
constexpr int32_t kMatchPadTerm = -(1 << 29);  // the offset term of a padding row or column

struct MatchPair {
    int64_t a_off, b_off;      // first descriptor of either frame in the call's descriptor block
    int64_t part_off;          // first triple of the pair's column partials [strips][n_b]
    int64_t row_off, col_off;  // first row / column of the pair in the per-row and per-column outputs of the launch
    int32_t n_a, n_b;
    int32_t strips, pad;
};

struct MatchItem {
    int32_t pair, strip;
};

struct MatchParams {
    float max_distance, max_ratio;
    int32_t mutual_best;
};

typedef int32_t match_i32x4 __attribute__((ext_vector_type(4)));

// in place: d ^= 0x80 per byte; off[d] = 128 * (sum of the flipped bytes as int8).  Eight threads per descriptor.
__global__ __launch_bounds__(kMatchThreads) void k_match_prep(uint8_t* __restrict__ desc, int32_t* __restrict__ off, int64_t n_desc) {
    const int64_t g = (int64_t)blockIdx.x * kMatchThreads + threadIdx.x;
    const int64_t d = g >> 3;
    const int part = (int)(g & 7);
    int32_t s = 0;
    if (d < n_desc) {
        uint4* p = reinterpret_cast<uint4*>(desc + d * xmatch::kDim) + part;
        uint4 v = *p;
        v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int b = 0; b < 4; ++b) s += (int32_t)(int8_t)(w[k] >> (8 * b));
        *p = v;
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (d < n_desc && part == 0) off[d] = 128 * s;
}

__device__ __forceinline__ xmatch::Top match_shfl_merge(const xmatch::Top& t, int mask) {
    xmatch::Top o;
    o.best = __shfl_xor(t.best, mask, 64);
    o.idx = __shfl_xor(t.idx, mask, 64);
    o.next = __shfl_xor(t.next, mask, 64);
    return xmatch::top_merge(t, o);
}

__global__ __launch_bounds__(kMatchThreads) void k_match_dots(
        const MatchItem* __restrict__ items, const MatchPair* __restrict__ pairs, const uint8_t* __restrict__ desc, const int32_t* __restrict__ off,
        int32_t* __restrict__ part, int32_t* __restrict__ row_top) {
    __shared__ __attribute__((aligned(16))) uint8_t Bs[kMatchCols * kMatchLdsRow];
    __shared__ int32_t Bterm[kMatchCols];
    __shared__ int32_t Cred[4 * kMatchCols * 3];
    const MatchItem it = items[blockIdx.x];
    const MatchPair pr = pairs[it.pair];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lcol = lane & 15, lgrp = lane >> 4;
    const int n_a = pr.n_a, n_b = pr.n_b;
    const uint8_t* __restrict__ A = desc + pr.a_off * xmatch::kDim;
    const uint8_t* __restrict__ B = desc + pr.b_off * xmatch::kDim;
    const int32_t* __restrict__ offA = off + pr.a_off;
    const int32_t* __restrict__ offB = off + pr.b_off;
    const int row0 = it.strip * kMatchStrip + wave * 32;        // first row of this wave

    // the A fragments of the two tiles and the offset terms of this lane's eight rows
    match_i32x4 af[2][2];
    int32_t rterm[2][4];
    xmatch::Top rtop[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int r = row0 + rt * 16 + lcol;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            af[rt][s] = match_i32x4{0, 0, 0, 0};
            if (r < n_a) af[rt][s] = *reinterpret_cast<const match_i32x4*>(A + (size_t)r * xmatch::kDim + (s * 4 + lgrp) * 16);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int rr = row0 + rt * 16 + lgrp * 4 + g;
            rterm[rt][g] = rr < n_a ? offA[rr] + (1 << 21) : kMatchPadTerm;
            rtop[rt][g] = xmatch::top_init();
        }
    }

    // staging: thread t carries 16-byte pieces t and t + 256 of the block's 512 (column = piece >> 3, part = piece & 7)
    const int n_blocks = (n_b + kMatchCols - 1) / kMatchCols;
    uint4 st[2];
    int32_t st_term = 0;
    auto fetch = [&](int cb) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int piece = tid + h * kMatchThreads, c = cb * kMatchCols + (piece >> 3);
            st[h] = make_uint4(0, 0, 0, 0);
            if (c < n_b) st[h] = *(reinterpret_cast<const uint4*>(B + (size_t)c * xmatch::kDim) + (piece & 7));
        }
        if (tid < kMatchCols) { const int c = cb * kMatchCols + tid; st_term = c < n_b ? offB[c] : kMatchPadTerm; }
    };
    auto stash = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int piece = tid + h * kMatchThreads;
            *reinterpret_cast<uint4*>(Bs + (piece >> 3) * kMatchLdsRow + (piece & 7) * 16) = st[h];
        }
        if (tid < kMatchCols) Bterm[tid] = st_term;
    };
    fetch(0);
    stash();
    __syncthreads();
#pragma unroll 1
    for (int cb = 0; cb < n_blocks; ++cb) {
        if (cb + 1 < n_blocks) fetch(cb + 1);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const uint8_t* bp = Bs + (ct * 16 + lcol) * kMatchLdsRow + lgrp * 16;
            const match_i32x4 b0 = *reinterpret_cast<const match_i32x4*>(bp), b1 = *reinterpret_cast<const match_i32x4*>(bp + 64);
            const int32_t cterm = Bterm[ct * 16 + lcol];
            const int32_t col = cb * kMatchCols + ct * 16 + lcol;
            xmatch::Top ctop = xmatch::top_init();
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                match_i32x4 acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[rt][0], b0, match_i32x4{0, 0, 0, 0}, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[rt][1], b1, acc, 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int32_t v = acc[g] + rterm[rt][g] + cterm;
                    xmatch::top_update(rtop[rt][g], v, col);
                    xmatch::top_update(ctop, v, row0 + rt * 16 + lgrp * 4 + g);
                }
            }
            ctop = match_shfl_merge(ctop, 16);
            ctop = match_shfl_merge(ctop, 32);
            if (lane < 16) {
                int32_t* q = Cred + (wave * kMatchCols + ct * 16 + lane) * 3;
                q[0] = ctop.best; q[1] = ctop.idx; q[2] = ctop.next;
            }
        }
        __syncthreads();                       // every wave has read Bs and written its column triples
        if (cb + 1 < n_blocks) stash();
        if (tid < kMatchCols) {
            const int c = cb * kMatchCols + tid;
            if (c < n_b) {
                xmatch::Top t{Cred[tid * 3], Cred[tid * 3 + 1], Cred[tid * 3 + 2]};
#pragma unroll
                for (int w = 1; w < 4; ++w) {
                    const int32_t* q = Cred + (w * kMatchCols + tid) * 3;
                    t = xmatch::top_merge(t, xmatch::Top{q[0], q[1], q[2]});
                }
                int32_t* o = part + (pr.part_off + (int64_t)it.strip * n_b + c) * 3;
                o[0] = t.best; o[1] = t.idx; o[2] = t.next;
            }
        }
        __syncthreads();                       // the next block is staged; Cred is free again
    }
    // the rows: merge across the 16 lanes that share a row
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            xmatch::Top t = rtop[rt][g];
            t = match_shfl_merge(t, 1);
            t = match_shfl_merge(t, 2);
            t = match_shfl_merge(t, 4);
            t = match_shfl_merge(t, 8);
            const int rr = row0 + rt * 16 + lgrp * 4 + g;
            if (lcol == 0 && rr < n_a) {
                int32_t* o = row_top + (pr.row_off + rr) * 3;
                o[0] = t.best; o[1] = t.idx; o[2] = t.next;
            }
        }
}

// counts [n_pairs][4]: matches, rows passing their test, columns passing theirs, 0
__global__ __launch_bounds__(kMatchThreads) void k_match_select(
        const MatchPair* __restrict__ pairs, MatchParams prm, const float* __restrict__ tab, const int32_t* __restrict__ part,
        const int32_t* __restrict__ row_top, int32_t* __restrict__ col_top, int32_t* col_match, int32_t* __restrict__ matches,
        int32_t* __restrict__ counts) {
    __shared__ int32_t wsum[4][2];
    const MatchPair pr = pairs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_a = pr.n_a, n_b = pr.n_b;
    int32_t* cm = col_match + pr.col_off;          // written, then read by other threads after the barrier: not restrict
    // columns: the partials in strip order, the test
    int32_t ncol = 0;
    for (int j = tid; j < n_b; j += kMatchThreads) {
        const int32_t* q = part + (pr.part_off + j) * 3;
        xmatch::Top t{q[0], q[1], q[2]};
        for (int s = 1; s < pr.strips; ++s) {
            q += (int64_t)n_b * 3;
            t = xmatch::top_merge(t, xmatch::Top{q[0], q[1], q[2]});
        }
        int32_t* o = col_top + (pr.col_off + j) * 3;
        o[0] = t.best; o[1] = t.idx; o[2] = t.next;
        const int32_t m = xmatch::match_of(tab, t, prm.max_distance, prm.max_ratio);
        cm[j] = m;
        ncol += m >= 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ncol += __shfl_xor(ncol, o, 64);
    if (lane == 0) wsum[wave][0] = ncol;
    __syncthreads();                           // cm is complete and visible to the workgroup
    ncol = wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0];
    __syncthreads();
    // rows in chunks of 256, ascending: the test, the mutual check, the compaction
    int32_t nrow = 0, base = 0;
    for (int i0 = 0; i0 < n_a; i0 += kMatchThreads) {
        const int i = i0 + tid;
        int32_t rm = -1;
        bool is = false;
        if (i < n_a) {
            const int32_t* q = row_top + (pr.row_off + i) * 3;
            rm = xmatch::match_of(tab, xmatch::Top{q[0], q[1], q[2]}, prm.max_distance, prm.max_ratio);
            is = xmatch::match_is(i, rm, cm, prm.mutual_best);
        }
        const unsigned long long bal = __ballot(is), balr = __ballot(rm >= 0);
        if (lane == 0) { wsum[wave][0] = __popcll(bal); wsum[wave][1] = __popcll(balr); }
        __syncthreads();
        int32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { before += w < wave ? wsum[w][0] : 0; total += wsum[w][0]; nrow += wsum[w][1]; }
        if (is) {
            const int32_t pos = base + before + __popcll(bal & ((1ull << lane) - 1ull));
            matches[(pr.row_off + pos) * 2] = i;
            matches[(pr.row_off + pos) * 2 + 1] = rm;
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) {
        int32_t* c = counts + 4 * (int64_t)blockIdx.x;
        c[0] = base; c[1] = nrow; c[2] = ncol; c[3] = 0;
    }
}

}  // namespace xba
