// acq_select.hip - the selection stage of the acquisition on gfx950 (MI355X): the rules that run after the ranking.
//
//   pp_acq_region_score_map     window impurity x window uncertainty: a score map for the ranking (pp_topk_select)
//   pp_spread_select            minimum pixel distance between the picks
//   pp_class_balance_select     round-robin over the predicted classes
//   pp_diverse_select           k-centre greedy over feature rows
//
// The three list selectors work on one object, written once below: the pool (PoolView: who is eligible), the fill phase of a short
// pool (pool_fill) and the arguments every entry checks (validate_pool).  A further selector is one kernel on top of these.
#include <cmath>

#include "pp_common.h"

namespace pp {

// ---- the pool: one image's rank-ordered candidate list cand[0 .. M) and the exclusion bytes of its N pixels -------------------------
// An entry is eligible when it lies in [0, N) and its exclusion byte is 0; for an entry outside [0, N) no byte is read (neither the
// exclusion byte nor whatever else a selector gathers at it).  Picks: idx / pos / n, at most kSpreadMaxK per image.
constexpr int kSpreadMaxK = 1024;

struct PoolView {
    const int32_t* cand;
    const uint8_t* excl;      // null: nothing is excluded
    int64_t M, N;
    __device__ __forceinline__ PoolView(const int32_t* cand_, const uint8_t* exclude, int64_t M_, int64_t N_, int64_t img)
        : cand(cand_ + img * M_), excl(exclude ? exclude + img * N_ : nullptr), M(M_), N(N_) {}
    __device__ __forceinline__ int at(int64_t i) const { return i < M ? cand[i] : -1; }       // beyond the list: -1, ineligible
    __device__ __forceinline__ bool inside(int c) const { return c >= 0 && (int64_t)c < N; }
    __device__ __forceinline__ int excl_byte(int c) const { return excl ? (int)excl[c] : 0; }  // of an entry inside [0, N)
    // 0: eligible.  The byte as loaded, not yet compared: a walk that asks a chunk ahead waits for the load only where it reads this
    __device__ __forceinline__ int blocked(int c) const
    {
        if (c < 0 || (int64_t)c >= N) return 1;
        return excl ? (int)excl[c] : 0;
    }
    __device__ __forceinline__ bool eligible(int c) const { return inside(c) && excl_byte(c) == 0; }
};

// The fill phase of a short pool, run by one wave: the list positions i (entry c) that take(i, c) names go, earliest first, to the
// output slots filled .. k - 1; also(slot) writes whatever else the selector keeps per pick.
template <typename Take, typename Also>
__device__ __forceinline__ void pool_fill(const PoolView& pool, int lane, int filled, int k, int32_t* out_idx, int32_t* out_pos, Take take,
                                          Also also)
{
    const uint64_t below = (1ull << lane) - 1ull;
    for (int64_t base = 0; base < pool.M && filled < k; base += kWave) {
        const int64_t i = base + lane;
        const int c = pool.at(i);
        const bool mine = i < pool.M && take(i, c);
        const uint64_t m = __ballot(mine);
        const int slot = filled + __popcll(m & below);
        if (mine && slot < k) {
            out_idx[slot] = c;
            out_pos[slot] = (int)i;
            also(slot);
        }
        filled += __popcll(m);
    }
}

// The arguments every list selector's entry takes; `who` names the entry in the message.  An entry checks its own arguments first.
static int validate_pool(const char* who, const int32_t* cand, int64_t B, int64_t M, int64_t N, int64_t k, const int32_t* out_idx,
                         const int32_t* out_pos, const int32_t* out_n)
{
    if (!cand) return fail(PP_ERR_BAD_ARG, "%s: cand is null", who);
    if (!out_idx) return fail(PP_ERR_BAD_ARG, "%s: out_idx is null", who);
    if (!out_pos) return fail(PP_ERR_BAD_ARG, "%s: out_pos is null", who);
    if (!out_n) return fail(PP_ERR_BAD_ARG, "%s: out_n is null", who);
    if (B < 1) return fail(PP_ERR_BAD_ARG, "%s: B=%lld < 1", who, (long long)B);
    if (N < 1 || N > 0x7FFFFFFFll) return fail(PP_ERR_BAD_ARG, "%s: N=%lld outside [1, 2^31 - 1]", who, (long long)N);
    if (M < 1 || M > N) return fail(PP_ERR_BAD_ARG, "%s: M=%lld outside [1, N=%lld]", who, (long long)M, (long long)N);
    if (k < 1 || k > M) return fail(PP_ERR_BAD_ARG, "%s: k=%lld outside [1, M=%lld]", who, (long long)k, (long long)M);
    if (k > kSpreadMaxK) return fail(PP_ERR_UNSUPPORTED, "%s: k=%lld > %d picks per image", who, (long long)k, kSpreadMaxK);
    if (B > 0x7FFFFFFFll) return fail(PP_ERR_UNSUPPORTED, "%s: B=%lld > 2^31 - 1 images per call", who, (long long)B);
    return PP_OK;
}

// ---- pp_spread_select: greedy minimum-distance selection over a rank-ordered candidate list -----------------------------
// One wave per image.  The accepted picks live in LDS as (y, x) pairs beside their list positions; the candidates are read 64 at a
// time (coalesced, the chunk after next already in flight, the exclusion bytes of the next chunk beside it).  Each lane tests its
// candidate against every pick accepted in earlier chunks (all lanes read the same LDS word: a broadcast); the survivors of the
// chunk are then resolved in rank order - ballot, the lowest live lane is accepted, its coordinates are handed to the live lanes,
// which drop out when they lie closer than d.  The wave leaves as soon as k picks are accepted; the fill phase is a second walk
// and runs only when the list ended first.  WIDE: squared distances in 64 bits (a coordinate difference may exceed 46340);
// otherwise H, W <= 32768 and 32 bits hold them.
struct SpreadParams {
    const int32_t* cand;      // [B,M]
    const uint8_t* exclude;   // [B,N] or null
    int32_t* out_idx;         // [B,k]
    int32_t* out_pos;         // [B,k]
    int32_t* out_n;           // [B]
    int64_t M, N;
    uint64_t d2;              // d * d (d clamped to 2^31 on the host: every distance in an image of < 2^31 pixels is smaller)
    int W, k;
};

template <bool WIDE>
__device__ __forceinline__ bool spread_far(int y, int x, int py, int px, uint64_t d2)
{
    if constexpr (WIDE) {
        const int64_t dy = (int64_t)y - py, dx = (int64_t)x - px;
        return (uint64_t)(dy * dy) + (uint64_t)(dx * dx) >= d2;
    } else {
        const int dy = y - py, dx = x - px;
        return (uint32_t)(dy * dy) + (uint32_t)(dx * dx) >= (uint32_t)d2;
    }
}

template <bool WIDE>
__global__ __launch_bounds__(kWave) void spread_select_kernel(SpreadParams p)
{
    __shared__ int2 s_pick[kSpreadMaxK];      // (y, x) of the accepted picks
    __shared__ int s_pos[kSpreadMaxK];        // their list positions, ascending
    const int lane = threadIdx.x;
    const int64_t img = blockIdx.x;
    const PoolView pool(p.cand, p.exclude, p.M, p.N, img);
    int32_t* out_idx = p.out_idx + img * p.k;
    int32_t* out_pos = p.out_pos + img * p.k;
    const int64_t M = p.M;
    const int k = p.k;
    auto load_c = [&](int64_t base) -> int { return pool.at(base + lane); };
    int n = 0;
    int c0 = load_c(0), c1 = load_c(kWave);
    int e0 = pool.blocked(c0);
    for (int64_t base = 0; base < M && n < k; base += kWave) {
        const int c2 = load_c(base + 2 * kWave);
        const int e1 = pool.blocked(c1);
        const int y = c0 / p.W, x = c0 - y * p.W;
        bool alive = e0 == 0;                 // (beyond the list: c0 = -1, ineligible)
        for (int j = 0; j < n; ++j) {
            const int2 q = s_pick[j];
            alive = alive && spread_far<WIDE>(y, x, q.x, q.y, p.d2);
        }
        uint64_t live = __ballot(alive);
        while (live != 0ull && n < k) {
            const int l = __ffsll((long long)live) - 1;
            const int py = __shfl(y, l, kWave), px = __shfl(x, l, kWave);
            if (lane == l) {
                s_pick[n] = make_int2(y, x);
                s_pos[n] = (int)(base + lane);
                out_idx[n] = c0;
                out_pos[n] = (int)(base + lane);
            }
            alive = alive && spread_far<WIDE>(y, x, py, px, p.d2);      // lane l itself: distance 0 < d * d
            live = __ballot(alive);
            ++n;
        }
        __syncthreads();                      // one wave: orders the LDS writes above before the next chunk's reads
        c0 = c1; e0 = e1; c1 = c2;
    }
    if (lane == 0) p.out_n[img] = n;
    if (n == k) return;
    // fill phase: the earliest list positions the spread phase did not accept, in list order, the distance rule dropped
    auto not_accepted = [&](int64_t i, int) -> bool {      // s_pos[0..n) ascends
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)s_pos[mid] < i) lo = mid + 1; else hi = mid;
        }
        return !(lo < n && (int64_t)s_pos[lo] == i);
    };
    pool_fill(pool, lane, n, k, out_idx, out_pos, not_accepted, [](int) {});
}

// ---- pp_acq_region_score_map: window impurity x window uncertainty (include/pixelpick_hip.h has the specification) -------
// One block per kRegionTH x kRegionTW tile of one image.  The (TH+2r) x (TW+2r) patch of label bins (u16; kRegionOut flags a position
// outside the image, nothing is clamped) and of u (0.0f outside: x + 0.0f == x, so the clipped window's sum is untouched) is staged
// once, a patch row per wave at a time.
// Window uncertainty: a separable pass.  A wave turns a patch row into its 64 row sums IN PLACE (lane l reads columns l .. l+2r and
// then writes column l: the wave's loads are all issued before its store, and no other wave touches the row), then each output
// sums 2r+1 of them; both sums run from their first term in a fixed order (no running sum: a NaN reaches exactly the windows that
// hold it).
// Impurity: the block's waves split the tile's rows; lane l of a wave owns column l and walks down its rows with the window's
// class counts in cnt[wave][bin][lane] (32-bit bins: the bank is the lane, no two lanes share a word).  The first window of a wave
// is built by 2r+1 row insertions; from then on a row leaves and a row enters, column by column as a PAIR: equal labels change
// nothing (inside a region of one label the step touches no count at all), different labels are two updates of different bins whose
// reads are in flight together.  Each update moves G = sum_c tab[n_c] by dtab[n] = tab[n+1] - tab[n] (exact integers, so the
// order of the walk cannot show in the result).  Per pixel that is at most 2(2r+1) updates whatever C is; C only sizes the
// counts, which the host fits into the CU's 160 KiB by the number of waves.
constexpr int kRegionTH = 64, kRegionTW = kWave, kRegionMaxR = 16, kRegionMaxWaves = 4;
constexpr size_t kRegionLdsMax = 160 * 1024;
constexpr uint32_t kRegionOut = 0xFFFFu;

struct RegionParams {
    const uint8_t* pred;      // [B,H,W]   (null in mode 2)
    const float* unc;         // [B,H,W]   (null in mode 1)
    const uint32_t* tab;      // [(2r+1)^2 + 1]   (null in mode 2)
    const uint8_t* exclude;   // [B,H,W] or null
    float* out;               // [B,H,W]
    int H, W, C, r, mode, flip, tiles_x, tiles_y, waves;
};

struct RegionLds {            // offsets in 32-bit words into the block's dynamic LDS
    int cnt, tab, dtab, u, lab;
    size_t bytes;
};

__host__ __device__ inline RegionLds region_lds(int C, int r, int mode, int waves)
{
    const int K = (2 * r + 1) * (2 * r + 1), PH = kRegionTH + 2 * r, PW = kRegionTW + 2 * r;
    const bool want_p = mode != 2, want_u = mode != 1;
    RegionLds l;
    int o = 0;
    l.cnt = o;  o += want_p ? waves * (C + 1) * kWave : 0;
    l.tab = o;  o += want_p ? K + 1 : 0;
    l.dtab = o; o += want_p ? K + 1 : 0;
    l.u = o;    o += want_u ? PH * PW : 0;
    l.lab = o;  o += want_p ? (PH * PW + 1) / 2 : 0;
    l.bytes = (size_t)o * 4;
    return l;
}

__global__ __launch_bounds__(kRegionMaxWaves * kWave) void region_score_kernel(RegionParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_region[];
    const RegionLds l = region_lds(p.C, p.r, p.mode, p.waves);
    const int r = p.r, D = 2 * r + 1, K = D * D, PH = kRegionTH + 2 * r, PW = kRegionTW + 2 * r;
    const int H = p.H, W = p.W, C = p.C;
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const bool want_p = p.mode != 2, want_u = p.mode != 1;
    uint32_t* s_cnt = s_region + l.cnt;
    uint32_t* s_tab = s_region + l.tab;
    uint32_t* s_dtab = s_region + l.dtab;
    float* s_u = reinterpret_cast<float*>(s_region + l.u);
    uint16_t* s_lab = reinterpret_cast<uint16_t*>(s_region + l.lab);

    int64_t t = blockIdx.x;
    const int tx = (int)(t % p.tiles_x);
    t /= p.tiles_x;
    const int ty = (int)(t % p.tiles_y);
    const int64_t img = (t / p.tiles_y) * ((int64_t)H * W);
    const int y0 = ty * kRegionTH, x0 = tx * kRegionTW;

    if (want_p) {
        for (int i = tid; i < p.waves * (C + 1) * kWave; i += nthr) s_cnt[i] = 0u;
        for (int i = tid; i <= K; i += nthr) {
            const uint32_t v = p.tab[i];
            s_tab[i] = v;
            s_dtab[i] = i < K ? p.tab[i + 1] - v : 0u;
        }
    }
    for (int pr = wave; pr < PH; pr += p.waves) {
        const int gy = y0 - r + pr;
        const bool row_in = gy >= 0 && gy < H;
        for (int pc = lane; pc < PW; pc += kWave) {
            const int gx = x0 - r + pc;
            const bool inside = row_in && gx >= 0 && gx < W;
            const int64_t g = img + (int64_t)gy * W + gx;
            if (want_p) {
                uint32_t b = kRegionOut;
                if (inside) {
                    const uint32_t v = p.pred[g];
                    b = v < (uint32_t)C ? v : (uint32_t)C;       // a byte >= C: the one extra bin
                }
                s_lab[pr * PW + pc] = (uint16_t)b;
            }
            if (want_u) {
                float u = 0.0f;
                if (inside) {
                    const float v = p.unc[g];
                    u = p.flip ? 1.0f - v : v;
                }
                s_u[pr * PW + pc] = u;
            }
        }
    }
    __syncthreads();
    if (want_u) {
        for (int pr = wave; pr < PH; pr += p.waves) {          // row sums in place: see the note above
            float* q = s_u + pr * PW + lane;
            float s = q[0];
            for (int j = 1; j < D; ++j) s += q[j];
            q[0] = s;
        }
        __syncthreads();
    }
    // no barrier below: a wave whose rows lie under the image leaves here
    const int rows = (kRegionTH + p.waves - 1) / p.waves;
    const int t0 = wave * rows;
    const int t1 = min(min(t0 + rows, kRegionTH), H - y0);
    if (t0 >= t1) return;
    const int x = x0 + lane;
    uint32_t* cnt = s_cnt + wave * (C + 1) * kWave + lane;
    uint32_t G = 0u;                                           // sum_c tab[n_c] of this lane's window
    // patch columns lane .. lane + 2r are the image columns x - r .. x + r; the next label is read while this one updates its count
    auto add_row = [&](int pr) {
        const uint16_t* q = s_lab + pr * PW + lane;
        uint32_t b = q[0];
        for (int j = 0; j < D; ++j) {
            const uint32_t bn = q[min(j + 1, D - 1)];
            if (b != kRegionOut) {
                uint32_t* c = cnt + b * kWave;
                const uint32_t n = *c;
                G += s_dtab[n];
                *c = n + 1u;
            }
            b = bn;
        }
    };
    auto slide = [&](int pl, int pe) {                         // patch row pl leaves the window, patch row pe enters it
        const uint16_t* ql = s_lab + pl * PW + lane;
        const uint16_t* qe = s_lab + pe * PW + lane;
        uint32_t bl = ql[0], be = qe[0];
        for (int j = 0; j < D; ++j) {
            const int jn = min(j + 1, D - 1);
            const uint32_t bln = ql[jn], ben = qe[jn];
            if (bl != be) {                                    // the same label (or both outside): counts and G stay
                if (bl != kRegionOut && be != kRegionOut) {    // two different bins: both reads in flight together
                    uint32_t* cl = cnt + bl * kWave;
                    uint32_t* ce = cnt + be * kWave;
                    const uint32_t nl = *cl - 1u, ne = *ce;
                    G += s_dtab[ne] - s_dtab[nl];
                    *cl = nl;
                    *ce = ne + 1u;
                } else if (bl != kRegionOut) {
                    uint32_t* cl = cnt + bl * kWave;
                    const uint32_t nl = *cl - 1u;
                    G -= s_dtab[nl];
                    *cl = nl;
                } else {
                    uint32_t* ce = cnt + be * kWave;
                    const uint32_t ne = *ce;
                    G += s_dtab[ne];
                    *ce = ne + 1u;
                }
            }
            bl = bln;
            be = ben;
        }
    };
    if (want_p)
        for (int pr = t0; pr <= t0 + 2 * r; ++pr) add_row(pr);
    for (int tr = t0; tr < t1; ++tr) {                         // output row y0 + tr: its window is patch rows tr .. tr + 2r
        const int y = y0 + tr;
        if (x < W) {
            const int ny = min(y + r, H - 1) - max(y - r, 0) + 1, nx = min(x + r, W - 1) - max(x - r, 0) + 1;
            const int N = ny * nx;
            float P = 0.0f, U = 0.0f;
            if (want_p) P = __fdiv_rn((float)(s_tab[N] - G), (float)(N << 16));
            if (want_u) {
                const float* q = s_u + tr * PW + lane;
                float s = q[0];
                for (int i = 1; i < D; ++i) s += q[i * PW];
                U = __fdiv_rn(s, (float)N);
            }
            float v = p.mode == 0 ? __fmul_rn(P, U) : p.mode == 1 ? P : U;
            const int64_t g = img + (int64_t)y * W + x;
            if (p.exclude && p.exclude[g] != 0) v = -1.0f;
            p.out[g] = v;
        }
        if (want_p && tr + 1 < t1) slide(tr, tr + 2 * r + 1);
    }
}

// ---- pp_class_balance_select: round-robin over the predicted classes of a rank-ordered pool (include/pixelpick_hip.h) ---
// One wave per image, spread_select_kernel's frame.  A pick's output slot is known without a sort: round r opens at slot
// S(r) = sum_c min(t_c, r) (t_c = the class totals), and inside a round the entries stand in list order - the order the list is
// walked in.  So:
//   walk 1   the class totals t_c in LDS (ds_add: integer sums, the same whatever order the lanes arrive in) and E; sixteen chunks of 64
//            candidates and their gathered bytes in flight (the walk is bound by the latency of the gather, the order does not matter here);
//   scans    D[v] = #{c : min(t_c, k) == v}, P = prefix(D), Q = prefix(P): S(r) = r T - Q[r-1] with T = P[k] the classes in the pool
//            (H[q] = T - P[q] classes reach round q).  s_next[r] = S(r), r = 0 .. k; R = the first r with S(r) >= n: rounds >= R hold no pick;
//   walk 2   in list order, 64 at a time: the rank inside the class from a ballot loop over the chunk's distinct classes (256 running
//            counters in LDS), then the slot s_next[r]++ from a ballot loop over the chunk's distinct rounds < R; an entry whose slot is
//            < n is written straight to the output.  Leaves as soon as n picks are out;
//   fill     only when E < k: a third walk hands the earliest ineligible positions the remaining slots.
constexpr int kBalanceUnroll = 16;

struct BalanceParams {
    const int32_t* cand;      // [B,M]
    const uint8_t* label;     // [B,N]
    const uint8_t* exclude;   // [B,N] or null
    int32_t* out_idx;         // [B,k]
    int32_t* out_pos;         // [B,k]
    int32_t* out_n;           // [B]
    int64_t M, N;
    int k;
};

// in-place inclusive prefix sum of a[0 .. L) by one wave: a run of consecutive entries per lane, the run totals scanned across lanes
__device__ __forceinline__ void balance_scan(uint32_t* a, int L, int lane)
{
    const int seg = (L + kWave - 1) / kWave;
    const int lo = min(lane * seg, L), hi = min(lo + seg, L);
    uint32_t s = 0;
    for (int i = lo; i < hi; ++i) s += a[i];
    uint32_t incl = s;
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += v;
    }
    uint32_t run = incl - s;
    for (int i = lo; i < hi; ++i) {
        run += a[i];
        a[i] = run;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kWave) void class_balance_kernel(BalanceParams p)
{
    __shared__ uint32_t s_cnt[256];                  // walk 1: class totals; walk 2: running class counts
    __shared__ uint32_t s_q[kSpreadMaxK + 1];        // D -> P -> Q
    __shared__ uint32_t s_next[kSpreadMaxK + 1];     // the next free output slot of round r
    const int lane = threadIdx.x;
    const int64_t img = blockIdx.x;
    const PoolView pool(p.cand, p.exclude, p.M, p.N, img);
    const uint8_t* label = p.label + img * p.N;
    int32_t* out_idx = p.out_idx + img * p.k;
    int32_t* out_pos = p.out_pos + img * p.k;
    const int64_t M = p.M;
    const int k = p.k;
    const uint64_t below = (1ull << lane) - 1ull;
    auto load_c = [&](int64_t base) -> int { return pool.at(base + lane); };
    // the class of an eligible candidate, -1 for an ineligible one (both bytes in flight together; beyond the list: c = -1)
    auto load_cls = [&](int c) -> int {
        if (!pool.inside(c)) return -1;
        const int e = pool.excl_byte(c);
        const int l = (int)label[c];
        return e == 0 ? l : -1;
    };

    for (int i = lane; i < 256; i += kWave) s_cnt[i] = 0u;
    for (int i = lane; i <= k; i += kWave) s_q[i] = 0u;
    __syncthreads();

    // walk 1: class totals and E
    int64_t E = 0;
    {
        int c[kBalanceUnroll];
#pragma unroll
        for (int u = 0; u < kBalanceUnroll; ++u) c[u] = load_c((int64_t)u * kWave);
        for (int64_t base = 0; base < M; base += kBalanceUnroll * kWave) {
            int nx[kBalanceUnroll], cl[kBalanceUnroll];
#pragma unroll
            for (int u = 0; u < kBalanceUnroll; ++u) nx[u] = load_c(base + (int64_t)(kBalanceUnroll + u) * kWave);
#pragma unroll
            for (int u = 0; u < kBalanceUnroll; ++u) cl[u] = load_cls(c[u]);
#pragma unroll
            for (int u = 0; u < kBalanceUnroll; ++u) {
                if (cl[u] >= 0) atomicAdd(&s_cnt[cl[u]], 1u);
                E += __popcll(__ballot(cl[u] >= 0));
                c[u] = nx[u];
            }
        }
    }
    __syncthreads();
    const int n = (int)(E < (int64_t)k ? E : (int64_t)k);
    if (lane == 0) p.out_n[img] = n;

    // scans: s_next[r] = S(r) = sum_c min(t_c, r), r = 0 .. k
    for (int c = lane; c < 256; c += kWave) {
        const uint32_t t = s_cnt[c];
        if (t != 0u) atomicAdd(&s_q[t < (uint32_t)k ? t : (uint32_t)k], 1u);
    }
    __syncthreads();
    for (int i = lane; i < 256; i += kWave) s_cnt[i] = 0u;      // from here on: the running counts of walk 2
    balance_scan(s_q, k + 1, lane);                  // P
    const uint32_t T = s_q[k];
    __syncthreads();
    balance_scan(s_q, k + 1, lane);                  // Q
    int R = k;
    for (int r = lane; r <= k; r += kWave) {
        const uint32_t S = r == 0 ? 0u : (uint32_t)r * T - s_q[r - 1];
        s_next[r] = S;
        if (S >= (uint32_t)n && r < R) R = r;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) R = min(R, __shfl_xor(R, off, kWave));
    __syncthreads();

    // walk 2: ranks, slots, picks
    int taken = 0;
    {
        int c0 = load_c(0), c1 = load_c(kWave);
        int cl0 = load_cls(c0);
        for (int64_t base = 0; base < M && taken < n; base += kWave) {
            const int c2 = load_c(base + 2 * kWave);
            const int cl1 = load_cls(c1);
            const bool el = cl0 >= 0;
            int r = 0;
            uint64_t todo = __ballot(el);
            while (todo != 0ull) {                   // one turn per distinct class of the chunk
                const int lc = __shfl(cl0, __ffsll((long long)todo) - 1, kWave);
                const bool mine = el && cl0 == lc;
                const uint64_t m = __ballot(mine);
                const uint32_t seen = s_cnt[lc];     // one word for all lanes: a broadcast
                if (mine) r = (int)(seen + (uint32_t)__popcll(m & below));
                if (lane == 0) s_cnt[lc] = seen + (uint32_t)__popcll(m);
                todo &= ~m;
            }
            const bool act = el && r < R;
            int slot = n;
            todo = __ballot(act);
            while (todo != 0ull) {                   // one turn per distinct round of the chunk
                const int lr = __shfl(r, __ffsll((long long)todo) - 1, kWave);
                const bool mine = act && r == lr;
                const uint64_t m = __ballot(mine);
                const uint32_t first = s_next[lr];
                if (mine) slot = (int)(first + (uint32_t)__popcll(m & below));
                if (lane == 0) s_next[lr] = first + (uint32_t)__popcll(m);
                todo &= ~m;
            }
            const bool pick = act && slot < n;       // the last round may be cut short
            if (pick) {
                out_idx[slot] = c0;
                out_pos[slot] = (int)(base + lane);
            }
            taken += __popcll(__ballot(pick));
            __syncthreads();                         // one wave: orders the LDS writes above before the next chunk's reads
            c0 = c1; cl0 = cl1; c1 = c2;
        }
    }
    if (n == k) return;
    // fill phase: the earliest ineligible list positions, in list order
    pool_fill(pool, lane, n, k, out_idx, out_pos, [&](int64_t, int c) { return !pool.eligible(c); }, [](int) {});
}

// ---- pp_diverse_select: k-centre greedy over the feature rows of a rank-ordered pool (include/pixelpick_hip.h) ------------------
// One block per image.  r_i = the squared distance of list position i to the nearest pick so far: kDivFar for an eligible position
// before the first pick (so pick 0 is the earliest eligible one by the tie rule alone), kDivDead for an ineligible or picked one.  A
// step is one pass over the image's candidates: r_i = min(r_i, D(i, last)), the best (r_i, smallest i) of a lane as the 64-bit key
// r << 32 | ~i, its maximum over the block by wave shuffles and one LDS round, the winner's row to s_last for the next step.  Eight
// candidates per thread are in flight against one broadcast read of s_last.  D = |a|^2 + |b|^2 - 2 a.b from packed byte dot products,
// exact in 32 bits (at most 256 * 255^2).
//   RES   the rows staged once as dword planes plane[j][i] (consecutive lanes read consecutive dwords: no bank conflict) with r behind
//         them, all k steps out of LDS;
//   else  rows and r (the caller's workspace) read from memory every step.
constexpr int kDivThreads = 1024;
constexpr int kDivChunk = 8;
constexpr uint32_t kDivDead = 0xFFFFFFFFu, kDivFar = 0x7FFFFFFFu;
constexpr size_t kDivLdsMax = 160 * 1024 - 1024;     // the dynamic part: the static arrays below take less than the 1 KiB left
#ifdef PP_DEBUG_KNOBS
bool g_diverse_stream = false;                       // test build: the streaming form at any M (pp_debug_set_acq_tuning, occ 11)
#else
constexpr bool g_diverse_stream = false;
#endif

struct DiverseParams {
    const int32_t* cand;      // [B,M]
    const uint32_t* feat;     // [B,M,ldw] dwords
    const uint8_t* exclude;   // [B,N] or null
    int32_t* out_idx;         // [B,k]
    int32_t* out_pos;         // [B,k]
    int32_t* out_dist;        // [B,k]
    int32_t* out_n;           // [B]
    uint32_t* r;              // [B,M] (streaming form)
    int64_t M, N;
    int ldw, dw;              // dwords per row: pitch, and those that hold features
    uint32_t tail_mask;       // of dword dw - 1
    int k;
};

__device__ __forceinline__ uint32_t dot4_u8(uint32_t a, uint32_t b, uint32_t acc)
{
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a, b, acc, false);
#else
    return acc + (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u) + (a >> 24) * (b >> 24);
#endif
}

template <bool RES>
__global__ __launch_bounds__(kDivThreads) void diverse_kernel(DiverseParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_div[];      // RES: plane[dw][M], then r[M]
    __shared__ uint32_t s_last[64];
    __shared__ uint32_t s_nb;
    __shared__ uint64_t s_red[kDivThreads / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
    const int64_t img = blockIdx.x;
    const int64_t M = p.M;
    const int dw = p.dw, ldw = p.ldw, k = p.k;
    const PoolView pool(p.cand, p.exclude, M, p.N, img);
    const int32_t* cand = pool.cand;
    const uint32_t* feat = p.feat + img * M * ldw;
    int32_t* out_idx = p.out_idx + img * k;
    int32_t* out_pos = p.out_pos + img * k;
    int32_t* out_dist = p.out_dist + img * k;
    uint32_t* r = RES ? s_div + (int64_t)dw * M : p.r + img * M;
    // dword j of row i, the bytes past F cleared
    auto word = [&](int64_t i, int j) -> uint32_t {
        if constexpr (RES) return s_div[(int64_t)j * M + i];
        else return feat[i * ldw + j] & (j == dw - 1 ? p.tail_mask : 0xFFFFFFFFu);
    };

    for (int64_t i = tid; i < M; i += kDivThreads) r[i] = pool.eligible(cand[i]) ? kDivFar : kDivDead;
    if constexpr (RES) {
        const int64_t words = M * ldw;
        for (int64_t e = tid; e < words; e += kDivThreads) {
            const int64_t i = e / ldw;
            const int j = (int)(e - i * ldw);
            if (j < dw) s_div[(int64_t)j * M + i] = feat[e] & (j == dw - 1 ? p.tail_mask : 0xFFFFFFFFu);
        }
    }
    __syncthreads();

    int n = 0;
    int64_t last = -1;
    for (; n < k; ++n) {
        uint64_t best = 0ull;
        const uint32_t nb = n > 0 ? s_nb : 0u;
        for (int64_t base = tid; base < M; base += (int64_t)kDivThreads * kDivChunk) {
            uint32_t rv[kDivChunk];
#pragma unroll
            for (int u = 0; u < kDivChunk; ++u) {
                const int64_t i = base + (int64_t)u * kDivThreads;
                rv[u] = i < M ? r[i] : kDivDead;
            }
            if (n > 0) {
                uint32_t aa[kDivChunk], ab[kDivChunk];
#pragma unroll
                for (int u = 0; u < kDivChunk; ++u) { aa[u] = 0u; ab[u] = 0u; }
                for (int j = 0; j < dw; ++j) {
                    const uint32_t b = s_last[j];
#pragma unroll
                    for (int u = 0; u < kDivChunk; ++u)
                        if (rv[u] != kDivDead) {
                            const uint32_t a = word(base + (int64_t)u * kDivThreads, j);
                            aa[u] = dot4_u8(a, a, aa[u]);
                            ab[u] = dot4_u8(a, b, ab[u]);
                        }
                }
#pragma unroll
                for (int u = 0; u < kDivChunk; ++u)
                    if (rv[u] != kDivDead) {
                        const int64_t i = base + (int64_t)u * kDivThreads;
                        rv[u] = i == last ? kDivDead : min(rv[u], nb + aa[u] - 2u * ab[u]);
                        r[i] = rv[u];
                    }
            }
#pragma unroll
            for (int u = 0; u < kDivChunk; ++u)
                if (rv[u] != kDivDead) {
                    const uint64_t key = ((uint64_t)rv[u] << 32) | (uint32_t)~(uint32_t)(base + (int64_t)u * kDivThreads);
                    best = key > best ? key : best;
                }
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), off, kWave);
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, off, kWave);
            const uint64_t o = ((uint64_t)hi << 32) | lo;
            best = o > best ? o : best;
        }
        if (lane == 0) s_red[wv] = best;
        __syncthreads();
        uint64_t win = 0ull;
#pragma unroll
        for (int v = 0; v < kDivThreads / kWave; ++v) win = s_red[v] > win ? s_red[v] : win;
        if (win == 0ull) break;                      // no eligible position is left (the same word in every thread)
        last = (int64_t)(~(uint32_t)win);
        if (tid == 0) {
            out_idx[n] = cand[last];
            out_pos[n] = (int)last;
            out_dist[n] = n == 0 ? -1 : (int)(uint32_t)(win >> 32);
        }
        if (tid < kWave) {                           // the winner's row and its squared norm for the next step
            const uint32_t b = tid < dw ? word(last, tid) : 0u;
            s_last[tid] = b;
            uint32_t nrm = dot4_u8(b, b, 0u);
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) nrm += (uint32_t)__shfl_xor((int)nrm, off, kWave);
            if (tid == 0) s_nb = nrm;
        }
        __syncthreads();
    }
    if (tid == 0) p.out_n[img] = n;
    if (n == k || tid >= kWave) return;
    // fill phase (one wave): the earliest ineligible list positions, in list order.  Fewer than k positions are eligible, so the
    // walk ends inside the first 2 k positions
    pool_fill(pool, lane, n, k, out_idx, out_pos, [&](int64_t, int c) { return !pool.eligible(c); }, [&](int slot) { out_dist[slot] = -1; });
}
}  // namespace pp

using namespace pp;

extern "C" {

int pp_spread_select(const int32_t* cand, int64_t B, int64_t M, int64_t W, int64_t N, int64_t k, int64_t d, const uint8_t* exclude,
                     int32_t* out_idx, int32_t* out_pos, int32_t* out_n, pp_stream_t stream)
{
    if (W < 1 || W > 0x7FFFFFFFll) return fail(PP_ERR_BAD_ARG, "spread_select: W=%lld outside [1, 2^31 - 1]", (long long)W);
    if (d < 1) return fail(PP_ERR_BAD_ARG, "spread_select: d=%lld < 1", (long long)d);
    if (int rc = validate_pool("spread_select", cand, B, M, N, k, out_idx, out_pos, out_n)) return rc;
    const int64_t H = cdiv(N, W);
    const bool wide = H > 32768 || W > 32768;
    // no two pixels of an image are 2^31 apart: a larger d selects the same picks.  32-bit form: dy^2 + dx^2 < 2^31
    uint64_t d2 = (uint64_t)(d < (1ll << 31) ? d : (1ll << 31));
    d2 *= d2;
    if (!wide && d2 > 0x80000000ull) d2 = 0x80000000ull;
    SpreadParams p{cand, exclude, out_idx, out_pos, out_n, M, N, d2, (int)W, (int)k};
    if (wide)
        hipLaunchKernelGGL(spread_select_kernel<true>, dim3((unsigned)B), dim3(kWave), 0, as_stream(stream), p);
    else
        hipLaunchKernelGGL(spread_select_kernel<false>, dim3((unsigned)B), dim3(kWave), 0, as_stream(stream), p);
    return check_launch("spread_select_kernel");
}

size_t pp_acq_region_table_words(int64_t r)
{
    return r < 1 || r > kRegionMaxR ? 0 : (size_t)((2 * r + 1) * (2 * r + 1) + 1);
}

int pp_acq_region_table(int64_t r, uint32_t* host_tab)
{
    if (!host_tab) return fail(PP_ERR_BAD_ARG, "region_table: host_tab is null");
    if (r < 1 || r > kRegionMaxR) return fail(PP_ERR_UNSUPPORTED, "region_table: r=%lld outside [1, %d]", (long long)r, kRegionMaxR);
    const int64_t K = (2 * r + 1) * (2 * r + 1);
    host_tab[0] = host_tab[1] = 0u;
    for (int64_t n = 2; n <= K; ++n) host_tab[n] = (uint32_t)llrint((double)n * log((double)n) * 65536.0);
    return PP_OK;
}

int pp_acq_region_score_map(const uint8_t* pred, const float* unc, int64_t B, int64_t C, int64_t H, int64_t W, int64_t r, int mode,
                            int flip, const uint32_t* tab, const uint8_t* exclude, float* out_map, pp_stream_t stream)
{
    if (mode < 0 || mode > 2) return fail(PP_ERR_BAD_ARG, "region_score_map: mode=%d outside 0..2", mode);
    if (!out_map) return fail(PP_ERR_BAD_ARG, "region_score_map: out_map is null");
    if (mode != 2 && !pred) return fail(PP_ERR_BAD_ARG, "region_score_map: pred is null (mode %d)", mode);
    if (mode != 2 && !tab) return fail(PP_ERR_BAD_ARG, "region_score_map: tab is null (mode %d)", mode);
    if (mode != 1 && !unc) return fail(PP_ERR_BAD_ARG, "region_score_map: unc is null (mode %d)", mode);
    if (B < 1) return fail(PP_ERR_BAD_ARG, "region_score_map: B=%lld < 1", (long long)B);
    if (H < 1) return fail(PP_ERR_BAD_ARG, "region_score_map: H=%lld < 1", (long long)H);
    if (W < 1) return fail(PP_ERR_BAD_ARG, "region_score_map: W=%lld < 1", (long long)W);
    if (C < 1 || C > 256) return fail(PP_ERR_BAD_ARG, "region_score_map: C=%lld outside [1, 256] (labels are bytes)", (long long)C);
    if (r < 1 || r > kRegionMaxR) return fail(PP_ERR_UNSUPPORTED, "region_score_map: r=%lld outside [1, %d]", (long long)r, kRegionMaxR);
    const int64_t i31 = 0x7FFFFFFFll;
    if (H > i31 / W) return fail(PP_ERR_UNSUPPORTED, "region_score_map: H*W=%lldx%lld > 2^31 - 1 pixels per image", (long long)H, (long long)W);
    const int64_t tiles_x = cdiv(W, kRegionTW), tiles_y = cdiv(H, kRegionTH);
    if (B > i31 / (tiles_x * tiles_y))
        return fail(PP_ERR_UNSUPPORTED, "region_score_map: B=%lld images of %lld tiles: a grid past 2^31 - 1 blocks", (long long)B,
                    (long long)(tiles_x * tiles_y));
    // the class counts take (C+1) * 256 B per wave: as many waves as fit beside the patch (C = 256, r = 16: one wave, 127 KiB)
    int waves = kRegionMaxWaves;
    while (waves > 1 && region_lds((int)C, (int)r, mode, waves).bytes > kRegionLdsMax) waves /= 2;
    const size_t lds_bytes = region_lds((int)C, (int)r, mode, waves).bytes;
    if (lds_bytes > kRegionLdsMax) return fail(PP_ERR_UNSUPPORTED, "region_score_map: %zu bytes of LDS", lds_bytes);
    if (lds_bytes > 64 * 1024) {                      // beyond the default dynamic-LDS limit of a launch: raise this kernel's (sticky, no sync)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(region_score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        (void)hipGetLastError();
    }
    RegionParams p{pred, unc, tab, exclude, out_map, (int)H, (int)W, (int)C, (int)r, mode, flip ? 1 : 0, (int)tiles_x, (int)tiles_y, waves};
    hipLaunchKernelGGL(region_score_kernel, dim3((unsigned)(B * tiles_x * tiles_y)), dim3(waves * kWave), lds_bytes, as_stream(stream), p);
    return check_launch("region_score_kernel");
}

int pp_class_balance_select(const int32_t* cand, int64_t B, int64_t M, int64_t N, int64_t k, const uint8_t* label, const uint8_t* exclude,
                            int32_t* out_idx, int32_t* out_pos, int32_t* out_n, pp_stream_t stream)
{
    if (!label) return fail(PP_ERR_BAD_ARG, "class_balance_select: label is null");
    if (int rc = validate_pool("class_balance_select", cand, B, M, N, k, out_idx, out_pos, out_n)) return rc;
    BalanceParams p{cand, label, exclude, out_idx, out_pos, out_n, M, N, (int)k};
    hipLaunchKernelGGL(class_balance_kernel, dim3((unsigned)B), dim3(kWave), 0, as_stream(stream), p);
    return check_launch("class_balance_kernel");
}

// the largest M the resident form of diverse_kernel takes: the planes of M rows and r behind them in the LDS one block may ask for
int64_t pp_diverse_resident_candidates(int64_t F)
{
    if (F < 1 || F > 256) return 0;
    return (int64_t)(kDivLdsMax / (4 * ((size_t)cdiv(F, 4) + 1)));
}

size_t pp_diverse_workspace_bytes(int64_t B, int64_t M, int64_t F)
{
    if (B < 1 || M < 1 || F < 1 || F > 256 || B > 0x7FFFFFFFll || M > 0x7FFFFFFFll || B * M > (1ll << 40)) return 0;
    return align_up((size_t)B * M * 4, 256);         // r, u32 [B,M]: read by the streaming form only
}

int pp_diverse_select(const int32_t* cand, int64_t B, int64_t M, int64_t N, int64_t k, const uint8_t* feat, int64_t F, int64_t ldf,
                      const uint8_t* exclude, int32_t* out_idx, int32_t* out_pos, int32_t* out_dist, int32_t* out_n, void* workspace,
                      size_t ws_bytes, pp_stream_t stream)
{
    if (!feat) return fail(PP_ERR_BAD_ARG, "diverse_select: feat is null");
    if (!out_dist) return fail(PP_ERR_BAD_ARG, "diverse_select: out_dist is null");
    if (!workspace) return fail(PP_ERR_BAD_ARG, "diverse_select: workspace is null");
    if (F < 1 || F > 256) return fail(PP_ERR_BAD_ARG, "diverse_select: F=%lld outside [1, 256]", (long long)F);
    if (ldf < F || ldf % 4 != 0 || ldf > 0x7FFFFFFFll)
        return fail(PP_ERR_BAD_ARG, "diverse_select: ldf=%lld must be a multiple of 4 and at least F=%lld", (long long)ldf, (long long)F);
    if (reinterpret_cast<uintptr_t>(feat) % 4 != 0) return fail(PP_ERR_BAD_ARG, "diverse_select: feat is not 4-byte aligned");
    if (int rc = validate_pool("diverse_select", cand, B, M, N, k, out_idx, out_pos, out_n)) return rc;
    if (B * M > (1ll << 40)) return fail(PP_ERR_UNSUPPORTED, "diverse_select: B*M=%lld list entries per call", (long long)(B * M));
    const size_t need = pp_diverse_workspace_bytes(B, M, F);
    if (ws_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 4 != 0)
        return fail(PP_ERR_BAD_ARG, "diverse_select: workspace of %zu bytes, %zu needed (4-byte aligned)", ws_bytes, need);
    const int dw = (int)cdiv(F, 4);
    const uint32_t tail = F % 4 ? (1u << (8 * (F % 4))) - 1u : 0xFFFFFFFFu;
    DiverseParams p{cand, reinterpret_cast<const uint32_t*>(feat), exclude, out_idx, out_pos, out_dist, out_n,
                    reinterpret_cast<uint32_t*>(workspace), M, N, (int)(ldf / 4), dw, tail, (int)k};
    hipStream_t st = as_stream(stream);
    if (M <= pp_diverse_resident_candidates(F) && !g_diverse_stream) {
        static bool attr_set = false;
        if (!attr_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(diverse_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)kDivLdsMax);
            attr_set = true;
        }
        hipLaunchKernelGGL(diverse_kernel<true>, dim3((unsigned)B), dim3(kDivThreads), (size_t)(dw + 1) * M * 4, st, p);
        return check_launch("diverse_resident_kernel");
    }
    hipLaunchKernelGGL(diverse_kernel<false>, dim3((unsigned)B), dim3(kDivThreads), 0, st, p);
    return check_launch("diverse_stream_kernel");
}
}  // extern "C"
