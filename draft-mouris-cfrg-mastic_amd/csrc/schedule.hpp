// Host-only launch plan of one chunk of a prep_init: which level kernels and
// binder sponges run, in what order, on which stream and after what.  Plain
// C++17, no HIP: mastic_hip.hip executes the plan (struct Chunk), and
// tests/host/schedule_host.cpp checks it on a CPU under ASan / UBSan.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "host_tree.hpp"
#include "params.hpp"

// ------------------------------------------------------------ shared constants
constexpr int NSLOT = 3;  // level buffers in flight between eval and absorb
constexpr int LAST_LEVEL_SEGMENTS_AUTO = 4;
// level_kernel.hpp EVAL_WAVES / EVAL_PROOF_WAVES and keccak.hpp KECCAK_RATE, which
// the kernels need as macros (mastic_hip.hip static_asserts that they agree)
constexpr int SCHED_EVAL_WAVES = 16;
constexpr int SCHED_EVAL_PROOF_WAVES = 8;
constexpr int SCHED_SPONGE_RATE = 168;  // bytes

// ------------------------------------------------------------------ the knobs
// The tuning fields of mastic_ctx that the schedule reads (mastic_ctx::k;
// MASTIC_EXPERIMENT_KNOBS builds and the mastic_set_* entry points write them).
// Every field changes the plan and tests/host/schedule_host.cpp sweeps each;
// the knobs whose A/B is settled are constants now (DESIGN.md "Retired knobs").
struct SchedKnobs {
    // Lanes per binder sponge.  Two (k_absorb_pair: half the dependent chain
    // per permutation, ~1.5x the VALU issue slots) while the chains are the
    // critical path, i.e. a chunk of few reports (C2's 16,384: one sponge wave
    // for every second SIMD); one (k_absorb: a third fewer VALU slots taken
    // from the level kernel beside it) once a chunk has enough reports for the
    // sponges to be throughput-bound (the 1M-report sweep's ~380k-report
    // chunks).  Same-box A/B (profiles/r05_v6_ab_single_lane_sponges.txt): one
    // lane is +4.5 % on the 1M sweep, -2 % on C2 and -21 % on C5 at 16,384.
    // 0 = by chunk size (>= absorb_single_min reports: one lane), 1 = always
    // one, 2 = always two (MASTIC_ABSORB_SINGLE).
    int absorb_mode = 0;
    size_t absorb_single_min = 65536;  // MASTIC_ABSORB_SINGLE_MIN
    int n_cus = 256;                     // compute units of the device
    // parent ranges of the last level of a cache-less single-stream miss (plan_chunk):
    // 0 = auto, k >= 1 forced (mastic_set_last_level_segments)
    int last_level_segments = 0;
    bool seg_balance = true;        // ... ranges of equal proofs per parent (MASTIC_SEG_BALANCE=0: equal parents)
    int split_sponges = -1;  // payload sponge a level earlier, on the third stream: -1 Field128 only, 0 never, 1 always (MASTIC_SPLIT_SPONGES)
    // the last level's node proofs in the level kernel, overlapped with its AES,
    // on cache hits and cache-on misses (MASTIC_FUSE_PROOFS=0: k_node_proof)
    bool fuse_proofs = true;
};

// ------------------------------------------------------------- level geometry
// Parents per wave: enough waves to fill 256 CUs several times over.
inline int choose_ppw(int n_parents, int groups) {
    long long per = (long long)n_parents * groups / 16384;
    return (int)std::max(1LL, std::min(per, 64LL));
}

// Parents per AES wave of the level kernel.  A level is one launch and the
// next level's launch waits for its last workgroup, so the workgroup count
// should fill whole rounds of the CUs (one workgroup per CU) with nearly full
// workgroups: pick, among 8..64 parents per wave, the count whose
// (work / (rounds x CUs)) is highest, preferring more parents per wave (fewer
// table fills) within 0.5 %.
inline int choose_eval_ppw(int n_parents, int groups, int aes_waves, int n_cus) {
    if ((long long)n_parents * groups < (long long)aes_waves * 8 * n_cus) return choose_ppw(n_parents, groups * 2);
    double best_eff = -1.0;
    int best = 64;
    for (int ppw = 64; ppw >= 8; ppw--) {
        const long long gy = (n_parents + (long long)aes_waves * ppw - 1) / ((long long)aes_waves * ppw);
        const long long rounds = (groups * gy + n_cus - 1) / n_cus;
        const double work = (double)groups * n_parents / ((double)aes_waves * ppw);
        const double eff = work / ((double)rounds * n_cus);
        if (eff > best_eff + 0.005) {
            best_eff = eff;
            best = ppw;
        }
    }
    return best;
}

// Items per parent at a small level (AesArgs::split).  A workgroup's 16
// waves share its items; a parent's AES is 2 extend blocks plus nblk convert
// blocks per child (next seed + payload: 2 + 2 nblk in lockstep pairs).  With
// few parents the launch time is the workgroup's longest serial chain:
// items per wave x blocks per item.  Pick the split minimising that (each
// item recomputes the extend pair; item 0 adds the next-seed pair), fewer
// items on ties.  At 16 or more parents this is 1 (no split).
// The proof waves first compute level l-1's node proofs (2 np_prev per
// report, spread over them; ~3 AES blocks of time per Keccak-p, the ratio
// miss_proof_waves uses) and then claim items from the same LDS counter, so
// the 16 waves' capacity is reduced by that head start.
inline void choose_split(int n_parents, int np_prev, int proof_waves, int nblk, int* split, int* split_blocks) {
    int best_k = 1, best_cost = 1 << 30;
    const int pw = std::max(1, proof_waves);
    const int proof_blocks = np_prev > 0 ? pw * ((2 * np_prev + pw - 1) / pw) * 3 : 0;
    for (int k = 1; k <= nblk; k++) {
        const int nb = (nblk + k - 1) / k;
        const int kk = (nblk + nb - 1) / nb;  // ranges actually non-empty
        if (kk != k) continue;
        const int chain = 2 + 2 * nb;
        // the items' waves: whole items per wave after the proof waves' head start
        const int per_wave =
            (n_parents * k * chain + proof_blocks + SCHED_EVAL_WAVES * chain - 1) / (SCHED_EVAL_WAVES * chain);
        const int cost = per_wave * chain + 2;
        if (cost < best_cost) {
            best_cost = cost;
            best_k = k;
        }
    }
    *split = best_k;
    *split_blocks = (nblk + best_k - 1) / best_k;
}

// Proof waves of a level kernel whose node proofs are fused and overlapped
// (a frontier-cache hit, level_kernel.hpp fuse_ovl): the proofs' share of the work
// per parent, two Keccak-p (VALU, ~3.2k CU-cycles) against the AES of the
// extend pair, the convert seeds, both children's payload blocks and the
// parent-payload recompute, 4 + 3 nblk blocks (LDS: 2 x 133 cycles per block
// at the kernel's ~50 % LDS efficiency).  C3 (Count): 7 of 16, the c2sweep
// (Sum 255, 9 payload blocks): 3.
// ... and of a miss's fused last level: per parent also the extend pair and,
// with no recompute, 3 + 2 nblk AES blocks; the proof waves also take level
// L-1's node proofs first (2 np[L-1] of them, spread over level L's parents).
inline int miss_proof_waves(const McParams& p, int np_prev, int np_last, bool has_prev) {
    const int epb = p.field == 64 ? 2 : 1;
    const int nblk = (p.value_len + epb - 1) / epb;
    const double proofs = 2.0 + (has_prev ? 2.0 * np_prev / std::max(1, np_last) : 0.0);
    const double K = 1585.0 * proofs, A = (4.0 + 2.0 * nblk) * 532.0;
    return std::max(1, std::min(12, (int)std::lround(SCHED_EVAL_WAVES * K / (K + A))));
}

inline int hit_proof_waves(const McParams& p) {
    const int epb = p.field == 64 ? 2 : 1;
    const int nblk = (p.value_len + epb - 1) / epb;
    const double K = 3170.0, A = (4.0 + 3.0 * nblk) * 532.0;
    return std::max(1, std::min(12, (int)std::lround(SCHED_EVAL_WAVES * K / (K + A))));
}

// Parent ranges [beg[q], beg[q + 1]) of a last level cut into k segments
// (plan_chunk).  A launch's proof waves get 2 n_parents[L-1] proofs in range 0
// and the previous range's 2 per parent after that.  The ranges shrink
// geometrically so that every launch has the same proofs per parent
// (s_0 = n_parents[L-1] y, s_q = s_{q-1} y, summing to n_parents[L]): the fixed
// split of a workgroup into AES and proof waves then fits each of them alike,
// and the last range -- whose proofs k_node_proof computes after the last
// level kernel -- is the smallest.  (Equal parents, or equal modelled AES +
// proof work with range 0 the smallest, measured slower:
// profiles/r08_v1_ab_last_level_segments.txt.)
inline std::vector<int> segment_ranges(const SchedKnobs& c, const TreeShape& t, int k) {
    const int npl = t.n_parents[t.L];
    std::vector<int> beg(k + 1, 0);
    beg[k] = npl;
    if (k <= 1) return beg;
    const double prev = (double)t.n_parents[t.L - 1];
    std::vector<double> sz(k, (double)npl / k);
    if (c.seg_balance) {
        double lo = 0.0, hi = 1.0 + (double)npl / prev;
        for (int it = 0; it < 60; it++) {
            const double y = 0.5 * (lo + hi);
            double sum = 0.0, last = prev;
            for (int q = 0; q < k; q++) {
                sz[q] = last * y;
                last = sz[q];
                sum += sz[q];
            }
            (sum < npl ? lo : hi) = y;
        }
    }
    // cumulative rounding; every range keeps at least one parent (k <= npl)
    double acc = 0.0;
    for (int q = 1; q < k; q++) {
        acc += sz[q - 1];
        beg[q] = std::max(beg[q - 1] + 1, std::min((int)std::lround(acc), npl - (k - q)));
    }
    return beg;
}

// Segments of the last level of a call that qualifies.  Forced
// (mastic_set_last_level_segments k >= 1): k, at most one range per parent.
// Auto: LAST_LEVEL_SEGMENTS_AUTO (the same-box A/B's pick), halved until every
// range's launch fills the CUs for at least two rounds of workgroups (each
// launch boundary drains the CUs and refills the tables: a small level gains
// nothing).
inline int last_level_segments(const SchedKnobs& c, const TreeShape& t, int groups, int par_waves) {
    const int np = t.n_parents[t.L];
    if (c.last_level_segments >= 1) return std::max(1, std::min(c.last_level_segments, np));
    int k = std::min(LAST_LEVEL_SEGMENTS_AUTO, np);
    for (; k > 1; k /= 2) {
        const std::vector<int> beg = segment_ranges(c, t, k);
        bool fills = true;
        for (int q = 0; q < k && fills; q++) {
            const int cnt = beg[q + 1] - beg[q];
            const int ppw = choose_eval_ppw(cnt, groups, par_waves, c.n_cus);
            const long long gy = (cnt + (long long)par_waves * ppw - 1) / ((long long)par_waves * ppw);
            fills = groups * gy >= 2LL * c.n_cus;
        }
        if (fills) break;
    }
    return std::max(1, k);
}

// ------------------------------------------------------------------- the plan
// Level-kernel instantiations (level_kernel.hpp eval_aes_body's GEN / FC / SPLIT /
// WIDE), as a bit set.  The legal ones: FC only with GEN and nothing else.
// (LV_PAY is not the plan's: the launch adds it to an FC launch whose input or
// output cache slot holds payloads-format nodes, memplan.hpp.)
enum LevelVariant : int { LV_GEN = 1, LV_FC = 2, LV_SPLIT = 4, LV_WIDE = 8, LV_PAY = 16 };
constexpr int LV_FC_PAY = LV_GEN | LV_FC | LV_PAY;
constexpr int LEVEL_VARIANTS[9] = {LV_GEN | LV_FC,
                                   0,       LV_GEN,           LV_SPLIT,           LV_GEN | LV_SPLIT,
                                   LV_WIDE, LV_WIDE | LV_GEN, LV_WIDE | LV_SPLIT, LV_WIDE | LV_GEN | LV_SPLIT};

// Stream roles: the main stream (level kernels), the chunk's sponge stream,
// and the ctx's third stream (payload sponges of the split / segmented forms).
enum StreamRole : int { ST_MAIN, ST_SPONGE, ST_THIRD };
// Timing of a sponge launch: none, the absorb pair of its step's event
// sextuple, or a sextuple of its own whose kernel pairs are empty.
enum SpongeMarks : int { MK_NONE, MK_STEP, MK_PIECE };

// A contiguous piece of a level's binder messages (a whole level, or a parent
// range of a segmented last level).
struct Piece {
    int node0, nodes;      // one-hot sponge: nodes [node0, node0 + nodes) of the level
    int parent0, parents;  // payload sponge: parents [parent0, parent0 + parents)
};

// Sponges which0 .. which0 + nwh - 1 (0 one-hot, 1 payload) over `piece` of
// `level`, on `stream` after step `after` (a launch's index; the final step is
// launches.size()) and after sponge launch `prev` (the same sponge's previous
// piece where that ran on another stream; -1: none).
struct SpongeLaunch {
    int level, which0, nwh;
    Piece piece;
    int stream, after, prev;
    int f_oh, f_pl;  // both fill positions on entry
    int marks;
};

// One level-kernel launch on the main stream: parents [p0, p0 + cnt) of
// `level`; its proof waves compute nodes [pv_node0, pv_node0 + pv_nodes) of
// pv_level.  wait_level >= 0: the launch reuses that level's ring slots and
// first waits for both of its sponges.  Its sponges: sponges[sp0, sp1).
struct LevelLaunch {
    int level, p0, cnt, variant;
    int split, split_blocks, ppw, gy, aes_waves, par_waves;
    int pv_level, pv_node0, pv_nodes, pv_npw;
    int fuse_proofs, wait_level, sp0, sp1;
};

struct ChunkPlan {
    bool pair, wide, split, fuse_last, seg_early;
    int nseg, last_stream;
    std::vector<LevelLaunch> launches;
    std::vector<SpongeLaunch> sponges;
    // the final step: k_node_proof over nodes [n0, n0 + nn) of level L, or
    // (fuse_last: nn = 0) marks only; then the last of `sponges`
    int final_n0, final_nn, final_npw;
    int f_oh, f_pl;         // fill positions for k_finalize
    int n_sync, n_timing;   // sync / timing events the chunk uses
};

// The schedule of one chunk of n reports.  cache: a frontier-cache slot
// exists; pipelined: the chunk's tail runs on its sponge stream, which may be
// the third stream (only a chunk that is not pipelined has the third stream
// to itself).  f_oh, f_pl: the fill positions of both sponges after their
// prefixes.  A hit plans level L only.
inline void plan_chunk(const SchedKnobs& k, const McParams& p, const TreeShape& t, int n, bool hit, bool cache,
                       bool pipelined, int f_oh, int f_pl, ChunkPlan* out) {
    ChunkPlan& P = *out;
    P.launches.clear();
    P.sponges.clear();
    const int L = t.L, wlw = p.value_len * p.w32, groups = (n + 63) / 64;  // report groups (rows beyond n are padding)
    const std::vector<int>& np = t.n_parents;
    P.pair = k.absorb_mode == 2 || (k.absorb_mode == 0 && (size_t)n < k.absorb_single_min);
    P.wide = P.pair;  // beside the 2-lane sponges the level kernel may take 104 VGPRs (k_eval_aes_wide)
    // Split schedule (single-chunk misses, MASTIC_SPLIT_SPONGES): level l's
    // payload differences are complete after eval(l), so its payload sponge
    // starts then, on the third stream, while its one-hot sponge still waits
    // for level l's node proofs (eval(l+1)'s proof waves).  The payload chain
    // -- the long one at C4 / C5 -- then runs a level earlier and leaves a
    // shorter tail after the last level.
    // Measured (profiles/r04_v23_ab_split_sponges.txt): C5 +1.4 %, C4 +0.6 %,
    // C2 -0.5 %, c2sweep -0.9 % -- so by default for Field128 only, whose
    // payload messages (VALUE_LEN x 16 B per parent) make that chain long.
    const bool split_on = k.split_sponges < 0 ? p.field == 128 : k.split_sponges > 0;
    P.split = split_on && !hit && !pipelined;
    // the last level's node proofs in the level kernel (after each workgroup's
    // parents) instead of a k_node_proof launch: cache hits, and a miss's
    // when the frontier cache is on (the sweeps: c2sweep +1 %, its level
    // kernels -4 %), not without it (C2 -1.7 %, C5 -0.9 %: the FC kernel's
    // 128 VGPRs leave no room for the previous level's sponge waves beside
    // it; profiles/r04_v21_ab_fused_last_miss.txt)
    P.fuse_last = k.fuse_proofs && (hit || cache);
    // The last level's sponges: on the main stream for a hit that runs as one
    // chunk (nothing to overlap them with: the next work on the main stream
    // needs them; the cross-stream event round trip cost ~0.08 ms per call),
    // else on the sponge stream after the level's earlier sponges.
    P.last_stream = (hit && !pipelined) ? ST_MAIN : ST_SPONGE;
    // items per workgroup: par_waves x ppw, par_waves = the AES waves (the
    // proof waves mop up after their proofs)
    const int par_waves = SCHED_EVAL_WAVES - SCHED_EVAL_PROOF_WAVES;
    // Segmented last level (mastic_set_last_level_segments): a miss with no
    // frontier cache, not pipelined, beside the 2-lane sponges.  Level L's
    // parents (BFS order, as are both binder messages) are cut into nseg
    // contiguous ranges, one level-kernel launch each.  The proof waves of
    // range 0 take level L-1's node proofs as ever; those of range q >= 1 the
    // proofs of level L's nodes of range q-1 (from cs_out, which the previous
    // launch wrote); k_node_proof is left with the last range's nodes.  The
    // sponges follow piece by piece -- payload piece q after launch q, one-hot
    // piece q-1 after launch q -- so that what remains after the last level
    // kernel is one range's proofs and sponge pieces instead of a level and a
    // half of them.  Every other call keeps one launch per level.
    P.nseg = 1;
    if (!cache && !hit && !pipelined && P.pair && !P.fuse_last)
        P.nseg = last_level_segments(k, t, groups, par_waves);
    // Levels L-1 and L then run the split form whatever the field: pay(L-1)
    // is complete after eval(L-1), so it goes to the third stream at once
    // (after absorb(L-2), which holds the payload sponge's previous piece)
    // instead of waiting, paired with oh(L-1), for eval(L)'s first proofs.
    P.seg_early = P.nseg > 1 && !P.split && L >= 2;
    const std::vector<int> seg_beg = segment_ranges(k, t, P.nseg);
    // a hit's levels 0..L-1 are cached: nothing is planned for them
    for (int lv = 0; hit && lv < L; lv++) {
        f_oh = (f_oh + 2 * np[lv] * 32) % SCHED_SPONGE_RATE;
        f_pl = (f_pl + (lv > 0 ? np[lv] * wlw * 4 : 0)) % SCHED_SPONGE_RATE;
    }
    int last[2] = {-1, -1};  // the latest launch of either sponge
    int pieces = 0;          // sponge launches with a timing sextuple of their own
    auto whole = [&](int lv) { return Piece{0, 2 * np[lv], 0, np[lv]}; };
    auto sponge = [&](int lv, int which0, int nwh, Piece pc, int stream, int marks) {
        SpongeLaunch s{lv, which0, nwh, pc, stream, (int)P.launches.size(), -1, f_oh, f_pl, marks};
        for (int w = which0; w < which0 + nwh; w++) {
            if (last[w] >= 0 && P.sponges[last[w]].stream != stream) s.prev = last[w];
            last[w] = (int)P.sponges.size();
        }
        if (which0 == 0) f_oh = (f_oh + pc.nodes * 32) % SCHED_SPONGE_RATE;
        if (which0 + nwh > 1) f_pl = (f_pl + (lv > 0 ? pc.parents * wlw * 4 : 0)) % SCHED_SPONGE_RATE;
        pieces += marks == MK_PIECE;
        P.sponges.push_back(s);
    };
    const int epb = p.field == 64 ? 2 : 1, nblk = (p.value_len + epb - 1) / epb;
    // Per level l, on two streams: the level kernel of level l (AES of level l
    // and the node proofs of level l-1) on the main stream, then the binder
    // sponges over level l-1's proofs and payload differences on the sponge
    // stream, so the sponges of one level overlap the evaluation of the next.
    for (int l = hit ? L : 0; l <= L; l++) {
        LevelLaunch a{};
        a.level = l;
        // small levels: parents split into block-range items (AesArgs::split);
        // not at the last level (out shares, frontier-cache staging) nor on a hit
        // (<= 32 parents: their pass-0 flags live in the workgroup's sync words)
        a.split = 1;
        a.split_blocks = nblk;
        if (!hit && l < L && np[l] <= 32)
            choose_split(np[l], l > 0 ? np[l - 1] : 0, SCHED_EVAL_PROOF_WAVES, nblk, &a.split, &a.split_blocks);
        const bool fuse = P.fuse_last && l == L;
        a.fuse_proofs = fuse ? 1 : 0;
        a.aes_waves = SCHED_EVAL_WAVES - SCHED_EVAL_PROOF_WAVES;
        if (fuse)
            a.aes_waves = SCHED_EVAL_WAVES -
                          (hit ? hit_proof_waves(p) : miss_proof_waves(p, np[l - 1 < 0 ? 0 : l - 1], np[l], l > 0));
        a.par_waves = par_waves;
        // the frontier-cache variant only where its features are used: the
        // last level (convert seeds staged for the cache) and a hit (parent
        // payloads recomputed, fused proofs); a miss's other levels run the
        // plain kernel (the variant's uniform branches and extra spills cost
        // a few per cent).  Beside the 2-lane sponges (96 VGPRs) the plain
        // variants take 104 (k_eval_aes_wide); beside k_absorb (128) they keep 96
        a.variant = ((cache && (hit || l == L)) || fuse)
                        ? LV_GEN | LV_FC
                        : (P.wide ? LV_WIDE : 0) | (a.split > 1 ? LV_SPLIT : 0) | (l == 0 || l == L ? LV_GEN : 0);
        const int nq = l == L ? P.nseg : 1;  // the segmented last level: one launch per parent range
        for (int q = 0; q < nq; q++) {
            a.wait_level = (!hit && l >= NSLOT && q == 0) ? l - NSLOT : -1;
            a.p0 = nq > 1 ? seg_beg[q] : 0;
            a.cnt = nq > 1 ? seg_beg[q + 1] - a.p0 : np[l];
            const int n_items = a.cnt * a.split;
            a.ppw = choose_eval_ppw(n_items, groups, par_waves, k.n_cus);
            // a split level keeps all items of a report group in one workgroup
            // (the fix-up pass needs every item of a parent stored): gy = 1
            if (a.split > 1) a.ppw = (n_items + par_waves - 1) / par_waves;
            a.gy = (n_items + a.par_waves * a.ppw - 1) / (a.par_waves * a.ppw);
            // range 0: level l-1's proofs (hit: they are cached); range q: those of range q-1
            const int pprev = q > 0 ? seg_beg[q - 1] : 0;
            a.pv_level = q > 0 ? l : l - 1;
            a.pv_node0 = 2 * pprev;
            a.pv_nodes = q > 0 ? 2 * (a.p0 - pprev) : (l > 0 && !hit) ? 2 * np[l - 1] : 0;
            const int pw = SCHED_EVAL_WAVES - a.aes_waves;  // proof waves of this launch
            a.pv_npw = (a.pv_nodes + a.gy * pw - 1) / (a.gy * pw);
            a.sp0 = (int)P.sponges.size();
            if (nq > 1) {
                // the one-hot piece whose proofs this launch made (range 0: level
                // L-1's, with its payload sponge unless that ran earlier) ...
                if (q > 0)
                    sponge(l, 0, 1, Piece{2 * pprev, 2 * (a.p0 - pprev), 0, 0}, ST_SPONGE, MK_STEP);
                else
                    sponge(l - 1, 0, (P.split || P.seg_early) ? 1 : 2, whole(l - 1), ST_SPONGE, MK_STEP);
                // ... and this range's payload piece
                sponge(l, 1, 1, Piece{0, 0, a.p0, a.cnt}, ST_THIRD, MK_PIECE);
            } else if (P.split && l > 0) {
                // payload(l) now, one-hot(l-1) after the proofs this launch made
                sponge(l, 1, 1, whole(l), ST_THIRD, MK_STEP);
                sponge(l - 1, 0, 1, whole(l - 1), ST_SPONGE, MK_NONE);
            } else if (l > 0 && !hit) {
                sponge(l - 1, 0, 2, whole(l - 1), ST_SPONGE, MK_STEP);
                // pay(L-1) is complete: on the third stream, after pay(L-2) in the launch above
                if (P.seg_early && l == L - 1) sponge(l, 1, 1, whole(l), ST_THIRD, MK_PIECE);
            }
            a.sp1 = (int)P.sponges.size();
            P.launches.push_back(a);
        }
    }
    // the last level's node proofs (a fused last level: the level kernel made
    // them; a segmented one: all but the last range's), then its sponges
    P.final_n0 = 2 * seg_beg[P.nseg - 1];
    P.final_nn = P.fuse_last ? 0 : 2 * np[L] - P.final_n0;
    P.final_npw = choose_ppw(P.final_nn, groups);
    sponge(L, 0, (P.nseg > 1 || P.split) ? 1 : 2, P.nseg > 1 ? Piece{P.final_n0, P.final_nn, 0, 0} : whole(L),
           P.last_stream, MK_STEP);
    P.f_oh = f_oh;
    P.f_pl = f_pl;
    // per launch and per sponge one event, the final step's, the FLP side stream's two
    P.n_sync = (int)(P.launches.size() + P.sponges.size()) + 1 + (t.weight_check ? 2 : 0);
    P.n_timing = 6 * ((int)P.launches.size() + 1 + pieces);
}
