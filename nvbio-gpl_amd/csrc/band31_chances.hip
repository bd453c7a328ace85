// band31_chances.hip -- the chances behind the band-31 end-to-end first pass, for gfx950: the gap chance (single jobs and pairs), the launch
// that runs it interleaved with the second chance, and the report of which jobs may pair.
#include "band31_ungapped_inl.h"

namespace nvbio_amd {

__global__ void __launch_bounds__(256)
gap_pairs_kernel(const BatchDev b, uint32_t* __restrict__ partner)
{
    const uint32_t job = blockIdx.x * 256u + threadIdx.x;
    const int role = gap_pair_role( b, job, job < b.n );
    if (job < b.n) partner[job] = role ? (role > 0 ? job + 1u : job - 1u) : 0xFFFFFFFFu;
}

// ---------------------------------------------------------------------------------------------
// The GAP chance (need_dp = 4: no diagonal of the window has few enough mismatches for the three chances above -- a read with an indel, its
// two candidate windows, four fifths of what used to reach the DP).  Same setting (SEMI_GLOBAL, match 0, one penalty P, plain gap terms,
// all 31 diagonals inside the text); with Cg(g) = -(open + (g-1) ext) the cost of a gap of g symbols, an alignment costs the sum of its gaps'
// Cg plus P per mismatch, and the classes of alignments are ordered by that cost.  EVALUATED exactly: ONE gap of g <= 5 symbols with e <= 2
// mismatches, by the lead / tail argument of the other chances taken to the third mismatch -- with lead_i(d) / tail_i(d) = the rows before
// the (i+1)-th / after the (i+1)-th-from-last mismatch of diagonal d, a text gap (prefix on d-g, suffix on d, ending in column d) with <= e
// mismatches exists iff lead_i(d-g) + tail_{e-i}(d) >= M for some i <= e, a pattern gap (prefix on d, suffix on d-g, ending in d-g) iff
// lead_i(d) + tail_{e-i}(d-g) + g >= M.  The minimum c* over all of them and the LARGEST end column among the members that reach it are the
// DP's optimum and BestSink's sink, PROVIDED no other alignment costs <= c*:
//   * ungapped: every diagonal has more than `cap` mismatches (why a need_dp = 4 job is here): >= (cap + 1) P.  A THIRD-CHANCE job (need_dp = 2)
//     brings its best diagonal instead (2 or 3 mismatches, U* and column stashed by the first pass): that class joins the evaluated ones with its
//     exact cost -P U* and its column, every other diagonal costs at least as much, and the term drops out of the bound;
//   * one gap with 3 mismatches, or of 6 symbols: Cg(1) + 3 P, Cg(6);  three gaps: 3 Cg(1);  two gaps and a mismatch: 2 Cg(1) + P;
//     two gaps of (1,3) / (2,2) or more: Cg(1) + Cg(3), 2 Cg(2)          -- c_unk = the least of these; c* < c_unk is required;
//   * two gaps of (1,1) or (1,2) / (2,1) symbols without a mismatch (costs 2 Cg(1), Cg(1) + Cg(2)): EXISTENCE is tested (over-approximated)
//     through the middle diagonal b as in the third chance: the prefix on a neighbour a may run to row lo, the suffix on a neighbour c may start
//     at row hi, a member exists iff lo >= hi or b has no mismatch in rows [lo, hi); one that costs <= c* sends the job to the DP.
// Anything else -- c* >= c_unk, no member at all, a two-gap member in reach -- is the DP's.  Over-approximation only ever costs a DP.
// ---------------------------------------------------------------------------------------------
// Not under a quality ramp.  Built and measured (members priced with the penalties their mismatching rows really carry, every split of them between
// prefix and suffix; parity green): with penalties 2..6 the cheapest class the kernel cannot see -- one gap and three mismatches at the SMALLEST
// penalty -- costs 14, so a job settles only while its optimum costs 13 or less; the third chance already takes U* >= -11 there, and on the robust
// batch the pass cost 1.1-1.7 ms for 0.5-1.0 ms of DP saved.  With the ladder taken to four priced mismatches per member (bound 18: two gaps and a
// mismatch; also built, also green) the DP went 3.9 -> 2.7 ms and the pass cost 2.1: a job costs the pass half a DP and only half of them settle.
// ONE walk for both shapes of gap-chance entry.  PAIR = false: the single job `job` (has_u: a third-chance job, need_dp = 2).
// PAIR = true: TWO jobs in one, `job` and job + 1, partners by gap_pair_role, both flagged 4 by the first pass -- the same read on the same
// strand, windows of M + 31 symbols that begin sh = 1 .. PAIR_MAX_SHIFT columns apart; the LOWER job is the one whose window begins first, the
// UPPER job the other (either may be `job`).  Diagonal d of the upper job IS diagonal D = d + sh of the lower one (the same rows against the
// same text symbols), so the read's planes are built once, the text's for the union window of M + 31 + sh symbols, and the 31 + sh diagonals
// D are walked once.  What a diagonal yields -- its first and last three mismatches -- does not depend on the job; which alignments COUNT
// does: a job's classes are those whose diagonals all lie in its own band, D in [0, 30] for the lower job, [sh, 30 + sh] for the upper.  Hence
// one set of accumulators per job (c* and the largest end column among the members that reach it -- columns relative to the job's own
// win_begin --, the two-gap existence bits), each fed at the job's own diagonal d = D resp. D - sh with its guards in the job's own numbering
// (d >= g, the middle diagonal's neighbours inside 0 .. 30).  The cost of a one-gap member is the same for both; the two-gap intervals differ
// only next to a band's edge and are otherwise evaluated once.  The single job is the pair's degenerate case: sh = 0, the lower job alone,
// diagonals 0 .. 32, 13 text words, and the third-chance join (below), which only it has.
// The wave-level gates are taken over every job's diagonals: they only ever skip tests whose outcome is known, so a wider gate changes no
// result.  Each job settles with c_unk_n (a flag-4 job: every diagonal of its own band has more than `cap` mismatches), a third-chance job
// with c_unk_u.
// The pair's text planes hold 224 bits and a funnel shift reaches 31: from D = 6 on they are kept 4 symbols down (the lowest diagonal still
// looked at is then the two-gap block's middle one, D - 2 >= 4), which keeps every shift within 0 .. 31 up to D = 35.
// Returns the flags (0: settled, scores / sinks written; 1: the DP's): bit 0 `job`'s, PAIR: bit 1 job + 1's.
template <int RBITS, bool PAIR>
__device__ __forceinline__ uint32_t
gap_chance_e2e31_walk(const BatchDev& b, const int32_t P, const GapLadder lad, const int32_t gap_open, const int32_t gap_ext,
                      int32_t* __restrict__ scores, uint2* __restrict__ sinks, const uint32_t job, const bool has_u)
{
    constexpr int NJ = PAIR ? 2 : 1;                             // accumulator sets: [0] the lower (or only) job, [1] the upper job
    const AlnJob   J = load_job( b, job );
    const uint32_t first = J.first, M = J.M;
    const bool     rev = J.rev, comp = J.comp;
    // (flagged by the first pass: 1 <= M <= 161, N >= M + 30 -- partners: both windows M + 31 symbols --, P > 0, open <= ext < 0)
    uint32_t tb = J.tb, up = 0u, sh = 0u;
    if constexpr (PAIR)
    {
        const uint32_t tb1 = b.win_begin[job + 1u];
        up = tb1 > tb ? 1u : 0u;                                 // which of the two is the upper job: job + up (the lower: job + 1 - up)
        sh = up ? tb1 - tb : tb - tb1;                           // 1 .. PAIR_MAX_SHIFT
        tb = up ? tb : tb1;
    }
    // c* and the largest end column among the members that reach it, as ONE number per job: cost << 6 | 63 - column
    // (columns <= 30; a member costs cg[g] + (i + j) P with g <= 5, i + j <= 2, and launch_pk runs only under packed_ok(), which holds every
    // penalty to 4096: costs stay below 2^15, the key needs them below 2^26 -- a wider limit there must be matched here): the least key is the
    // least cost and, among equals, the largest column, as BestSink's `<=`
    uint32_t best_key[NJ];
    #pragma unroll
    for (int j = 0; j < NJ; ++j) best_key[j] = 0xFFFFFFFFu;
    auto take = [&](const int j, const int32_t c, const uint32_t end) {
        const uint32_t key = ((uint32_t)c << 6) | (63u - end);
        best_key[j] = key < best_key[j] ? key : best_key[j];
    };
    // need_dp = 2: a third-chance job -- its best diagonal (2 or 3 mismatches) is in scores / sinks; that ungapped class joins the evaluated ones
    if (!PAIR && has_u) take( 0, -scores[job], sinks[job].x - M );

    PlaneWords pw;
    {
        uint64_t rlo[3], rhi[3], rn[3], tlo[4], thi[4];
        ReadWords<RBITS> rw;
        load_read_words<RBITS>( b.reads, first, M, rw );
        // (b.text_planes is wave-uniform; the pair's union window: 5 units, see load_text_units)
        TextUnits<PAIR ? 5 : 4> tu;
        if (b.text_planes) load_text_units<PAIR ? 5 : 4>( b.text_planes, tb, tu );
        else if constexpr (PAIR) load_text_words<14>( b.text, tb, M + 31u + sh, tu );
        else
        {
            const uint32_t N = b.win_end[job] - tb;
            load_text_words<13>( b.text, tb, N < 192u ? N : 192u, tu );
        }
        read_planes192<RBITS>( rw, first, M, rev, comp, rlo, rhi, rn );
        if (b.text_planes) text_planes_units<PAIR ? 5 : 4>( tu, tb, tlo, thi );
        else if constexpr (PAIR) text_planes_words<14>( tu, tb, tlo, thi );
        else text_planes_words<13>( tu, tb, tlo, thi );
        pw.set( rlo, rhi, rn, tlo, thi, M );
    }

    // the cost ladder
    constexpr int GA = GAP_CHANCE_GA;
    int32_t cg[GA + 1];                                          // cg[g] = cost of a gap of g symbols
    #pragma unroll
    for (int g = 1; g <= GA; ++g) cg[g] = -(gap_open + (g - 1) * gap_ext);
    const int32_t c_unk = (!PAIR && has_u) ? lad.c_unk_u : lad.c_unk_n;     // (every OTHER diagonal of a job that brings its best one costs at least c_unk_u)
    const int32_t cost11 = 2 * cg[1], cost12 = cg[1] + cg[2];

    // the read's LAST 32 rows (rows base .. base + 31; all of them if it has fewer) and the text symbols they can meet, as words of their own:
    // bit j of (plT, phT, pnT, pmT) = row base + j, bit j of (qlT, qhT) = text symbol base + j
    const uint32_t base = M >= 32u ? M - 32u : 0u;
    const uint32_t bw = base >> 5, bs = base & 31u;
    uint32_t plT, phT, pnT, pmT, qlT[2], qhT[2];
    {
        uint32_t a[4] = { 0, 0, 0, 0 }, c[4] = { 0, 0, 0, 0 };
        #pragma unroll
        for (int k = 0; k < 6; ++k)
            if (bw == (uint32_t)k)
            {
                a[0] = pw.pl[k]; a[1] = k + 1 < 6 ? pw.pl[k + 1] : 0u; a[2] = pw.ph[k]; a[3] = k + 1 < 6 ? pw.ph[k + 1] : 0u;
                c[0] = pw.pn[k]; c[1] = k + 1 < 6 ? pw.pn[k + 1] : 0u; c[2] = pw.pm[k]; c[3] = k + 1 < 6 ? pw.pm[k + 1] : 0u;
            }
        plT = __builtin_amdgcn_alignbit( a[1], a[0], bs ); phT = __builtin_amdgcn_alignbit( a[3], a[2], bs );
        pnT = __builtin_amdgcn_alignbit( c[1], c[0], bs ); pmT = __builtin_amdgcn_alignbit( c[3], c[2], bs );
    }
    // (the text's two words: 64 symbols from `base` on in the planes as they stand -- taken again when the pair's planes move down, see D == 6 below)
    auto tail_text = [&]() {
        uint32_t t[3] = { 0, 0, 0 }, u[3] = { 0, 0, 0 };
        #pragma unroll
        for (int k = 0; k < 6; ++k)
            if (bw == (uint32_t)k)
            {
                t[0] = pw.ql[k]; t[1] = k + 1 < 7 ? pw.ql[k + 1] : 0u; t[2] = k + 2 < 7 ? pw.ql[k + 2] : 0u;
                u[0] = pw.qh[k]; u[1] = k + 1 < 7 ? pw.qh[k + 1] : 0u; u[2] = k + 2 < 7 ? pw.qh[k + 2] : 0u;
            }
        qlT[0] = __builtin_amdgcn_alignbit( t[1], t[0], bs ); qlT[1] = __builtin_amdgcn_alignbit( t[2], t[1], bs );
        qhT[0] = __builtin_amdgcn_alignbit( u[1], u[0], bs ); qhT[1] = __builtin_amdgcn_alignbit( u[2], u[1], bs );
    };
    tail_text();
    // history of the last GA diagonals (slot k: diagonal D - 1 - k): (lead0, lead1, lead2) and (tail0, tail1, tail2) packed a byte each (<= 161)
    uint32_t Lp[GA], Tp[GA];
    #pragma unroll
    for (int k = 0; k < GA; ++k) { Lp[k] = 0; Tp[k] = 0; }
    // three histories of the last diagonals in one word, a byte each: bit k = diagonal D - 1 - k could be half of a one-gap alignment (`hot`) /
    // bit 8 + k = it is `long` / bit 16 + k = it has NO `mid` (the two-gap gate, below)
    uint32_t hist = 0;
    bool ex11[NJ], ex12[NJ];
    #pragma unroll
    for (int j = 0; j < NJ; ++j) { ex11[j] = false; ex12[j] = false; }
    const int32_t Mi = (int32_t)M;
    // lead_i(a) + tail_j(c) + g >= M with g <= GA needs one of the two at least (M - GA) / 2: only such diagonals are looked at pair by pair
    const int32_t hot_thr = (Mi - GA) / 2;
    uint32_t xo = 0;                                             // the planes stand xo symbols down

    // no mismatch of the diagonal x symbols on in rows [lo, hi)?  (lo >= hi: an empty middle segment -- counted as a member.)  bf / bl: its third
    // mismatch from either end (first / last if it has fewer): nearly always one of them lies inside and no word is looked at
    auto clean = [&](const uint32_t x, const int32_t bf, const int32_t bl, const int32_t lo, const int32_t hi) -> bool {
        if (lo >= hi) return true;
        if ((bf >= lo && bf < hi) || (bl >= lo && bl < hi)) return false;
        bool any = false;
        #pragma unroll
        for (int k = 0; k < 6; ++k)
        {
            const int32_t a0 = lo - 32 * k > 0 ? lo - 32 * k : 0, a1 = hi - 32 * k < 32 ? hi - 32 * k : 32;
            if (a0 < a1)
            {
                const uint32_t hi_m = (a1 >= 32) ? 0xFFFFFFFFu : ((1u << a1) - 1u);
                const uint32_t lo_m = (1u << a0) - 1u;
                any = any || ((pw.mmw( k, x ) & hi_m & ~lo_m) != 0u);
            }
        }
        return !any;
    };

    for (uint32_t D = 0; D <= 32u + (PAIR ? PAIR_MAX_SHIFT : 0u); ++D)
    {
        if constexpr (PAIR)
        {
            if (!__any( D <= 32u + sh )) break;                  // (wave-uniform: the largest shift of the wave's pairs)
            if (D == 6u)
            {
                #pragma unroll
                for (int k = 0; k < 6; ++k)
                {
                    pw.ql[k] = __builtin_amdgcn_alignbit( pw.ql[k + 1], pw.ql[k], 4u );
                    pw.qh[k] = __builtin_amdgcn_alignbit( pw.qh[k + 1], pw.qh[k], 4u );
                }
                pw.ql[6] >>= 4; pw.qh[6] >>= 4;
                tail_text();
                xo = 4u;
            }
        }
        const uint32_t x = D - xo;                               // <= 31
        const bool have = D <= 30u + sh;                         // a diagonal of the (union) window
        const int32_t dU = (int32_t)D - (int32_t)sh;             // this diagonal in the upper job's numbering
        const bool haveL = D <= 30u;                             // ... of the lower job's own band (the upper one's: 0 <= dU <= 30)
        // the first three and the last three mismatching rows of diagonal D.  A diagonal that is not the read's own (or its partner across the
        // indel) holds three mismatches in its first 32 and in its last 32 rows: those two words decide, branch-free; only where some lane of
        // the wave found fewer are the words walked from both ends, as far as some lane still needs
        uint32_t f0 = M, f1 = M, f2 = M, l0 = 0xFFFFFFFFu, l1 = 0xFFFFFFFFu, l2 = 0xFFFFFFFFu;
        bool mid_d = false;
        if (have)
        {
            uint32_t w = pw.mmw( 0, x );
            if (w) { f0 = (uint32_t)__builtin_ctz( w ); w &= w - 1u; }
            if (w) { f1 = (uint32_t)__builtin_ctz( w ); w &= w - 1u; }
            if (w) f2 = (uint32_t)__builtin_ctz( w );
            const uint32_t tl = __builtin_amdgcn_alignbit( qlT[1], qlT[0], x ), th = __builtin_amdgcn_alignbit( qhT[1], qhT[0], x );
            w = (((plT ^ tl) | (phT ^ th)) & pmT) | pnT;          // rows base .. base + 31
            if (w) { const uint32_t t = 31u - (uint32_t)__builtin_clz( w ); l0 = base + t; w &= ~(1u << t); }
            if (w) { const uint32_t t = 31u - (uint32_t)__builtin_clz( w ); l1 = base + t; w &= ~(1u << t); }
            if (w) l2 = base + 31u - (uint32_t)__builtin_clz( w );
            mid_d = M >= 96u && pw.mmw( 1, x ) != 0u;            // a mismatch in rows 32 .. 63, all of them rows of the read and below its last 32
        }
        if (__any( have && M > 32u && (f2 == M || l2 == 0xFFFFFFFFu) ))
        {
            f0 = f1 = f2 = M; l0 = l1 = l2 = 0xFFFFFFFFu;
            #pragma unroll
            for (int k = 0; k < 6; ++k)
                if (__any( have && f2 == M && pw.pm[k] != 0u ))
                {
                    uint32_t w = (have && f2 == M) ? pw.mmw( k, x ) : 0u;
                    if (f0 == M && w) { f0 = 32u * k + (uint32_t)__builtin_ctz( w ); w &= w - 1u; }
                    if (f0 != M && f1 == M && w) { f1 = 32u * k + (uint32_t)__builtin_ctz( w ); w &= w - 1u; }
                    if (f1 != M && f2 == M && w) f2 = 32u * k + (uint32_t)__builtin_ctz( w );
                }
            #pragma unroll
            for (int k = 5; k >= 0; --k)
                if (__any( have && l2 == 0xFFFFFFFFu && pw.pm[k] != 0u ))
                {
                    uint32_t w = (have && l2 == 0xFFFFFFFFu) ? pw.mmw( k, x ) : 0u;
                    if (l0 == 0xFFFFFFFFu && w) { const uint32_t t = 31u - (uint32_t)__builtin_clz( w ); l0 = 32u * k + t; w &= ~(1u << t); }
                    if (l0 != 0xFFFFFFFFu && l1 == 0xFFFFFFFFu && w) { const uint32_t t = 31u - (uint32_t)__builtin_clz( w ); l1 = 32u * k + t; w &= ~(1u << t); }
                    if (l1 != 0xFFFFFFFFu && l2 == 0xFFFFFFFFu && w) l2 = 32u * k + 31u - (uint32_t)__builtin_clz( w );
                }
        }
        const int32_t L0 = (int32_t)f0, L1 = (int32_t)f1, L2 = (int32_t)f2;          // rows before the 1st / 2nd / 3rd mismatch
        const int32_t T0 = l0 == 0xFFFFFFFFu ? Mi : Mi - 1 - (int32_t)l0;             // rows after the last / last-but-one / last-but-two
        const int32_t T1 = l1 == 0xFFFFFFFFu ? Mi : Mi - 1 - (int32_t)l1;
        const int32_t T2 = l2 == 0xFFFFFFFFu ? Mi : Mi - 1 - (int32_t)l2;
        const bool hot_d = have && (L2 >= hot_thr || T2 >= hot_thr);
        const bool long_d = have && (L0 >= 30 || T0 >= 30);

        if (__any( have && (hot_d || (hist & 31u) != 0u) ))
        {
            #pragma unroll
            for (int g = 1; g <= GA; ++g)
                if (have && D >= (uint32_t)g && (hot_d || ((hist >> (g - 1)) & 1u)))
                {
                    // the member's two diagonals D - g and D lie in the lower job's band iff D <= 30, in the upper one's iff D - g >= sh
                    const bool inL = haveL, inU = PAIR && dU >= g;
                    const int32_t a0 = (int32_t)(Lp[g - 1] & 255u), a1 = (int32_t)((Lp[g - 1] >> 8) & 255u), a2 = (int32_t)(Lp[g - 1] >> 16);
                    const int32_t t0 = (int32_t)(Tp[g - 1] & 255u), t1 = (int32_t)((Tp[g - 1] >> 8) & 255u), t2 = (int32_t)(Tp[g - 1] >> 16);
                    // the cheapest member of a gap of g with a prefix of `lead` rows, a suffix of `tail` rows and `more` rows between them
                    auto cheapest = [&](const int32_t (&lead)[3], const int32_t (&tail)[3], const int32_t more) -> int32_t {
                        int32_t c = 0x7FFFFFFF;
                        #pragma unroll
                        for (int i = 0; i <= 2; ++i)
                            #pragma unroll
                            for (int j = 0; i + j <= 2; ++j)
                                if (lead[i] + tail[j] + more >= Mi)
                                {
                                    const int32_t v = cg[g] + (i + j) * P;
                                    c = v < c ? v : c;
                                }
                        return c;
                    };
                    // text gap of g: diagonal D - g (prefix), then D (suffix); ends in column D
                    if (a2 + T2 >= Mi)
                    {
                        const int32_t lead[3] = { a0, a1, a2 }, tail[3] = { T0, T1, T2 };
                        const int32_t c = cheapest( lead, tail, 0 );
                        if (c != 0x7FFFFFFF)
                        {
                            if (inL) take( 0, c, D );
                            if constexpr (PAIR) if (inU) take( 1, c, (uint32_t)dU );
                        }
                    }
                    // pattern gap of g: diagonal D (prefix), then D - g (suffix); ends in column D - g
                    if (L2 + t2 + g >= Mi)
                    {
                        const int32_t lead[3] = { L0, L1, L2 }, tail[3] = { t0, t1, t2 };
                        const int32_t c = cheapest( lead, tail, g );
                        if (c != 0x7FFFFFFF)
                        {
                            if (inL) take( 0, c, D - (uint32_t)g );
                            if constexpr (PAIR) if (inU) take( 1, c, (uint32_t)(dU - g) );
                        }
                    }
                }
        }
        // two gaps around the middle diagonal D - 2 (history slot 1): neighbours D - 4 (slot 3), D - 3 (slot 2), D - 1 (slot 0), D (this diagonal).
        // For the lower job it is its diagonal bm = D - 2 at its iterations d = D in 2 .. 32, for the upper one bm = dU - 2 at d = dU in 2 .. 32;
        // a neighbour counts iff it lies in the job's band.
        // THE GATE.  Each test below asks whether bm is clean on [lo, hi) with lo <= lead0(a) + 2 and hi >= M - tail0(c) - 2 for neighbours a, c
        // of bm.  If no neighbour is `long` (lead0 >= 30 or tail0 >= 30) then lo <= 31 and hi >= M - 31; if besides bm has a `mid` (M >= 96 and a
        // mismatch in rows 32 .. 63) then M - 31 >= 65, so lo < hi, rows 32 .. 63 lie inside [lo, hi) and bm is NOT clean there: all three tests
        // are false and ex11 / ex12 stay as they are.  The block is skipped for a diagonal where that holds for EVERY lane of the wave: an
        // unrelated diagonal has its first and last mismatch within a few rows of the ends and one in any 32 rows, so only the diagonals
        // around some lane's own ones (and those of the few lanes with M < 96) still run it.  Nothing is approximated: a skipped test is a
        // test whose outcome is known to be "no member".
        const bool actL = D >= 2u && D <= 32u, actU = PAIR && dU >= 2 && dU <= 32;
        if (__any( (actL || actU) && (long_d || (hist & 0x20D00u) != 0u) ))        // `long`: slots 0, 2, 3 or this diagonal; no `mid`: slot 1
        {
            const int32_t NEG = -(1 << 20), POS = 1 << 20;
            // the intervals of a job whose iteration this is d (its middle diagonal d - 2), hv: its diagonal d exists
            auto intervals = [&](const int32_t d, const bool hv, int32_t (&iv)[4]) {
                const int32_t bm = d - 2;
                iv[0] = NEG; iv[1] = POS; iv[2] = NEG; iv[3] = POS;                      // lo1, hi1, lo2, hi2
                if (bm >= 1)       { iv[0] = (int32_t)(Lp[2] & 255u); iv[1] = Mi - (int32_t)(Tp[2] & 255u) - 1; }      // a = bm - 1: text gap in; c = bm - 1: pattern gap out
                if (bm + 1 <= 30)  { const int32_t p = (int32_t)(Lp[0] & 255u) + 1, q = Mi - (int32_t)(Tp[0] & 255u); iv[0] = p > iv[0] ? p : iv[0]; iv[1] = q < iv[1] ? q : iv[1]; }
                if (bm >= 2)       { iv[2] = (int32_t)(Lp[3] & 255u); iv[3] = Mi - (int32_t)(Tp[3] & 255u) - 2; }      // a / c = bm - 2
                if (hv)            { const int32_t p = L0 + 2, q = Mi - T0; iv[2] = p > iv[2] ? p : iv[2]; iv[3] = q < iv[3] ? q : iv[3]; }   // a / c = bm + 2
            };
            // the middle diagonal's third mismatch from either end (first / last if it has fewer): a row that is NOT clean
            const int32_t b2 = (int32_t)(Lp[1] >> 16), b1 = (int32_t)((Lp[1] >> 8) & 255u), b0 = (int32_t)(Lp[1] & 255u);
            const int32_t bf = b2 < Mi ? b2 : (b1 < Mi ? b1 : b0);
            const int32_t e2 = (int32_t)(Tp[1] >> 16), e1 = (int32_t)((Tp[1] >> 8) & 255u), e0 = (int32_t)(Tp[1] & 255u);
            const int32_t et = e2 < Mi ? e2 : (e1 < Mi ? e1 : e0);
            const int32_t bl = et < Mi ? Mi - 1 - et : NEG;
            const uint32_t xm = x - 2u;                            // the middle diagonal in the planes as they stand (D >= 2 here)
            auto tests = [&](const int32_t (&iv)[4], bool& r11, bool& r12) {
                r11 = false; r12 = false;
                if (iv[0] > NEG && iv[1] < POS) r11 = clean( xm, bf, bl, iv[0], iv[1] );
                if (iv[0] > NEG && iv[3] < POS) r12 = clean( xm, bf, bl, iv[0], iv[3] );
                if (iv[2] > NEG && iv[1] < POS) r12 = r12 || clean( xm, bf, bl, iv[2], iv[1] );
            };
            int32_t iv[4];
            bool r11 = false, r12 = false;
            if (actL)
            {
                intervals( (int32_t)D, haveL, iv );
                tests( iv, r11, r12 );
                ex11[0] = ex11[0] || r11; ex12[0] = ex12[0] || r12;
            }
            if constexpr (PAIR)
                if (actU)
                {
                    // away from a band's edge the two jobs ask the same questions: all four neighbours of the middle diagonal lie in both bands
                    // iff dU - 2 >= 2 (the upper job's lower edge) and D <= 30 (the lower job's upper edge)
                    if (!(actL && dU >= 4 && D <= 30u))
                    {
                        intervals( dU, dU <= 30, iv );
                        tests( iv, r11, r12 );
                    }
                    ex11[1] = ex11[1] || r11; ex12[1] = ex12[1] || r12;
                }
        }
        // shift the history
        #pragma unroll
        for (int k = GA - 1; k > 0; --k) { Lp[k] = Lp[k - 1]; Tp[k] = Tp[k - 1]; }
        Lp[0] = (uint32_t)L0 | ((uint32_t)L1 << 8) | ((uint32_t)L2 << 16);
        Tp[0] = (uint32_t)T0 | ((uint32_t)T1 << 8) | ((uint32_t)T2 << 16);
        hist = ((hist << 1) & 0xFEFEFEu) | (hot_d ? 1u : 0u) | (long_d ? 0x100u : 0u) | (mid_d ? 0u : 0x10000u);
    }
    uint32_t flags = 0;
    #pragma unroll
    for (int j = 0; j < NJ; ++j)
    {
        const int32_t  best_cost = best_key[j] == 0xFFFFFFFFu ? 0x7FFFFFFF : (int32_t)(best_key[j] >> 6);
        const uint32_t best_end  = 63u - (best_key[j] & 63u);
        const bool settled = best_cost < c_unk && !(ex11[j] && cost11 <= best_cost) && !(ex12[j] && cost12 <= best_cost);
        const uint32_t which = j ? up : (PAIR ? 1u - up : 0u);   // 0: `job`, 1: job + 1
        if (settled) { scores[job + which] = -best_cost; sinks[job + which] = make_uint2( M + best_end, M ); }
        else flags |= 1u << which;
    }
    return flags;
}

// the single job (has_u: a third-chance job, need_dp = 2): returns its flag
template <int RBITS>
__device__ __forceinline__ uint32_t
gap_chance_e2e31_job(const BatchDev& b, const int32_t P, const GapLadder lad, const int32_t gap_open, const int32_t gap_ext,
                     int32_t* __restrict__ scores, uint2* __restrict__ sinks, const uint32_t job, const bool has_u)
{
    return gap_chance_e2e31_walk<RBITS,false>( b, P, lad, gap_open, gap_ext, scores, sinks, job, has_u );
}

// the pair `job`, job + 1: returns the two flags
template <int RBITS>
__device__ __forceinline__ uint32_t
gap_chance_e2e31_pair(const BatchDev& b, const int32_t P, const GapLadder lad, const int32_t gap_open, const int32_t gap_ext,
                      int32_t* __restrict__ scores, uint2* __restrict__ sinks, const uint32_t job)
{
    return gap_chance_e2e31_walk<RBITS,true>( b, P, lad, gap_open, gap_ext, scores, sinks, job, false );
}

// one workgroup's chunks of list `pairs` (slot0 < n = the list's length): every pair through gap_chance_e2e31_pair, the members it does not
// settle on out.dp
template <int RBITS>
__device__ __forceinline__ void
gap_chance_pairs_chunks(const BatchDev& b, const int32_t P, const GapLadder lad, const int32_t gap_open, const int32_t gap_ext,
                        int32_t* __restrict__ scores, uint2* __restrict__ sinks, uint8_t* __restrict__ need_dp,
                        const uint32_t* __restrict__ list_p, const uint32_t n, const uint32_t slot0, const JobLists& out, JobAppendTwo::Lds& lds)
{
    JobAppendTwo app;
    auto job_of = [&](const int k, const int r) -> uint32_t { return list_p[slot0 + 256u * k + threadIdx.x] + (uint32_t)r; };
    #pragma unroll 1
    for (int k = 0; k < JOB_LIST_CHUNKS; ++k)
    {
        uint32_t flags = 0;
        if (slot0 + 256u * k + threadIdx.x < n)
        {
            const uint32_t job = job_of( k, 0 );
            flags = gap_chance_e2e31_pair<RBITS>( b, P, lad, gap_open, gap_ext, scores, sinks, job );
            need_dp[job] = (uint8_t)(flags & 1u); need_dp[job + 1u] = (uint8_t)(flags >> 1);
        }
        app.note( lds, k, (flags & 1u) != 0u, (flags & 2u) != 0u );
    }
    app.flush( lds, out, job_of );
}

// the jobs of job_list, then the pairs of list_p (launched over one workgroup more than the whole batch's: those behind the lists' ends leave
// before they touch anything); one that ends as 1 goes on out.dp
template <int RBITS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5)))
gap_chance_e2e31_kernel(const BatchDev b, const int32_t P, const GapLadder lad, const int32_t gap_open, const int32_t gap_ext,
                        int32_t* __restrict__ scores, uint2* __restrict__ sinks, uint8_t* __restrict__ need_dp,
                        const uint32_t* __restrict__ job_list, const uint32_t* __restrict__ job_count,
                        const uint32_t* __restrict__ list_p, const uint32_t* __restrict__ count_p, const JobLists out)
{
    __shared__ JobAppend<1>::Lds s_lists;
    __shared__ JobAppendTwo::Lds s_two;
    constexpr uint32_t W = 256u * JOB_LIST_CHUNKS;
    const uint32_t n = *job_count, np = *count_p;
    const uint32_t nbp = (np + W - 1u) / W;                          // the pairs' workgroups come first: they run the longest
    if (blockIdx.x < nbp)
    {
        gap_chance_pairs_chunks<RBITS>( b, P, lad, gap_open, gap_ext, scores, sinks, need_dp, list_p, np, blockIdx.x * W, out, s_two );
        return;
    }
    const uint32_t slot0 = (blockIdx.x - nbp) * W;
    if (slot0 >= n) return;                                          // (the whole workgroup)
    JobAppend<1> app;
    auto job_of = [&](const int k) -> uint32_t { return job_list[slot0 + 256u * k + threadIdx.x]; };
    #pragma unroll 1
    for (int k = 0; k < JOB_LIST_CHUNKS; ++k)
    {
        int which = -1;
        if (slot0 + 256u * k + threadIdx.x < n)
        {
            const uint32_t job  = job_of( k );
            const uint32_t flag = gap_chance_e2e31_job<RBITS>( b, P, lad, gap_open, gap_ext, scores, sinks, job, need_dp[job] == 2 );
            need_dp[job] = (uint8_t)flag;
            if (flag) which = 0;
        }
        app.note( s_lists, k, which );
    }
    app.flush( s_lists, out, job_of );
}

// BOTH chances in one launch: the second chance (list_s) waits for lines in scans of divergent depth, the gap chance (list_t) is bound by VALU
// issue, neither reads what the other writes (each job is on one list; both only append to out.dp), so the wave slots and issue cycles one
// leaves idle are the other's.  A workgroup has ONE role, taken from blockIdx.x: with nb2 / nb3 workgroups' worth of jobs on the two lists,
// workgroup i is the second chance's iff floor( (i + 1) nb2 / (nb2 + nb3) ) > floor( i nb2 / (nb2 + nb3) ) -- an even interleave, nb2 such
// workgroups among the first nb2 + nb3, spread over the gap chance's whole duration -- and walks chunk floor( i nb2 / (nb2 + nb3) ) of its
// list (the gap chance's: i minus that).  The jobs run the device functions of the two separate launches, so every job ends as it does there.
// The gap chance's role has two lists: the pairs of list_p (gap_chance_e2e31_pair; a workgroup holds pairs only, so no wave runs both device
// functions) and the single jobs of list_t; with nbp workgroups' worth of pairs the role's first nbp workgroups take the pairs, which run
// the longest.
// (Launched over job_list_grid( b.n ) + 2 workgroups -- the lists are disjoint and a pair stands for two jobs, so nb2 + nb3 + nbp <= that --;
// those past nb2 + nb3 + nbp leave at once.)
template <int RBITS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5)))
chances_e2e31_kernel(const BatchDev b, const int32_t P, const int32_t G, const GapLadder lad, const int32_t gap_open, const int32_t gap_ext,
                     int32_t* __restrict__ scores, uint2* __restrict__ sinks, uint8_t* __restrict__ need_dp,
                     const uint32_t* __restrict__ list_s, const uint32_t* __restrict__ count_s,
                     const uint32_t* __restrict__ list_t, const uint32_t* __restrict__ count_t,
                     const uint32_t* __restrict__ list_p, const uint32_t* __restrict__ count_p, const JobLists out)
{
    __shared__ JobAppend<1>::Lds s_lists;
    __shared__ JobAppendTwo::Lds s_two;
    constexpr uint32_t W = 256u * JOB_LIST_CHUNKS;
    const uint32_t n2 = *count_s, n3 = *count_t, np = *count_p;
    const uint32_t nb2 = (n2 + W - 1u) / W, nbp = (np + W - 1u) / W, nb3 = (n3 + W - 1u) / W + nbp, nb = nb2 + nb3;     // (n2, n3, np < 2^31: no overflow)
    if (blockIdx.x >= nb) return;                                    // (the whole workgroup)
    const uint32_t before = (uint32_t)((uint64_t)blockIdx.x * nb2 / nb);                 // second-chance workgroups in front of this one
    const bool     second = (uint32_t)((uint64_t)(blockIdx.x + 1u) * nb2 / nb) > before;
    if (!second && blockIdx.x - before < nbp)
    {
        gap_chance_pairs_chunks<RBITS>( b, P, lad, gap_open, gap_ext, scores, sinks, need_dp, list_p, np, (blockIdx.x - before) * W, out, s_two );
        return;
    }
    const uint32_t n      = second ? n2 : n3;
    const uint32_t* __restrict__ job_list = second ? list_s : list_t;
    const uint32_t slot0  = (second ? before : blockIdx.x - before - nbp) * W;           // < n: this role has a chunk left (see above)
    JobAppend<1> app;
    auto job_of = [&](const int k) -> uint32_t { return job_list[slot0 + 256u * k + threadIdx.x]; };
    #pragma unroll 1
    for (int k = 0; k < JOB_LIST_CHUNKS; ++k)
    {
        int which = -1;
        if (slot0 + 256u * k + threadIdx.x < n)
        {
            const uint32_t job  = job_of( k );
            const uint32_t flag = second ? ungapped_e2e31_job<RBITS,1,false>( b, P, G, gap_open, gap_ext, scores, sinks, job, nullptr )
                                         : gap_chance_e2e31_job<RBITS>( b, P, lad, gap_open, gap_ext, scores, sinks, job, need_dp[job] == 2 );
            need_dp[job] = (uint8_t)flag;
            if (flag) which = 0;
        }
        app.note( s_lists, k, which );
    }
    app.flush( s_lists, out, job_of );
}

nvbio_status launch_gap_chance_e2e31(const uint32_t rbits, const bool with_second, const BatchDev& b, const SchemeDev& sc, const int32_t P, const int32_t G,
                                     const GapLadder lad, int32_t* scores, uint2* sinks, uint8_t* need_dp, const JobLists& out, hipStream_t s)
{
    return with_value( ReadBits31(), (int)rbits, [&](auto RB)
    {
        if (with_second)
            return NVB_LAUNCH( (chances_e2e31_kernel<RB>), dim3( job_list_grid( b.n ) + 2u ), dim3( 256 ), s, b, P, G, lad, sc.pat_go, sc.pat_ge, scores, sinks, need_dp,
                               (const uint32_t*)out.second, out.count( JOB_SECOND ), (const uint32_t*)out.third, out.count( JOB_THIRD ),
                               (const uint32_t*)out.pairs, out.count( JOB_PAIRS ), out );
        return NVB_LAUNCH( (gap_chance_e2e31_kernel<RB>), dim3( job_list_grid( b.n ) + 1u ), dim3( 256 ), s, b, P, lad, sc.pat_go, sc.pat_ge, scores, sinks, need_dp,
                           (const uint32_t*)out.third, out.count( JOB_THIRD ), (const uint32_t*)out.pairs, out.count( JOB_PAIRS ), out );
    }, [&] { return invalid_bits( rbits, 2u ); } );
}

nvbio_status launch_gap_pairs(const BatchDev& b, uint32_t* partner, hipStream_t s)
{
    return NVB_LAUNCH( gap_pairs_kernel, dim3( (b.n + 255u) / 256u ), dim3( 256 ), s, b, partner );
}

} // namespace nvbio_amd
