// band31_ungapped_inl.h -- one job of the band-31 end-to-end first pass and of its second / third chance.  Inlined by two units: the first
// pass and its list passes (band31_first_pass.hip) and the fused chances launch for the second chance (band31_chances.hip, MODE 1).  The
// first pass is pinned to 72 registers: whatever this file changes, or what it includes, changes that kernel.
#pragma once
#include "band31_jobs.h"

namespace nvbio_amd {

// ---------------------------------------------------------------------------------------------
// Ungapped shortcut for end-to-end (SEMI_GLOBAL) scoring with match = 0 (nvBowtie's default mode).
// Every alignment with at least one gap scores at most G = max(pattern gap open, text gap open) < 0: nothing
// else in it can be positive.  The ungapped alignments are the 31 diagonals of the band, diagonal d scoring
// U_d = -P * (number of rows i with read[i] != text[i+d]) for a constant mismatch penalty P.  Hence, if
// U* = max over the reportable end columns d of U_d is > G, the DP's optimum is U*, the last row holds U* in
// exactly the columns with U_d = U*, and BestSink's "last maximum wins" picks the largest such d -- all known
// from 31 shifted XOR + popcounts over bit planes, about an eighth of the DP's instructions.  Jobs with
// U* <= G (two or more mismatches at -6/-8, or an indel) are flagged and go through the DP unchanged.
// Reportable end columns: d = 0 always, d >= 1 iff d < min(M+30, N) - (M-1) (gotoh_banded_inl.h:631-643); such
// diagonals lie inside the text, so the band-31 cache quirk for symbols past the text end never touches them.
// ---------------------------------------------------------------------------------------------
// THIRD = false: the pass over every job (first and second chance); a job that neither settles but whose U* a third chance could
//   still settle (see below) gets need_dp = 2.
// THIRD = true : the pass over the list of those jobs (job_list / job_count on the device), which resolves each to 0 or 1.
//   Kept apart because the third chance is ten times the work of the rest and only one job in eight needs it: inside the first
//   pass every wave paid for it (measured: 0.39 -> 2.1 ms per launch), on a dense list it costs what it saves several times over.
// MODE 0: the pass over every job: best diagonal, settled or not; a job the second (third) chance could still settle is flagged
//   need_dp = 3 (2) with its best diagonal stashed in scores / sinks -- those checks cost as much as everything else in this pass and
//   every wave paid for them whenever one lane needed one (the second chance, one job in four, was HALF of this kernel's 1.46 ms).
// MODE 1 / 2: the pass over the dense list of the need_dp = 3 / 2 jobs (job_list / job_count on the device): the second / third chance,
//   each job ends as 0 or 1.
// QUAL (MODE 0 only): the mismatch penalty depends on the row's base quality (nvBowtie's default ramp, scoring.h:73-92), P = the
//   scheme's SMALLEST penalty (> 0).  U_d = -(sum of the penalties of diagonal d's mismatching rows) lies between -pmax c_d and
//   -P c_d for c_d mismatches, so only diagonals with P c_d <= pmax min_d c_d can hold the maximum: those few (the read's own diagonal,
//   its partners across an indel) are summed exactly, row by row, from the quality bytes; every other diagonal is ruled out by its
//   count alone.  Everything after that -- which classes of gapped alignments could still reach U* -- is argued with P as the least a
//   mismatch can cost, which only makes the classes larger (more jobs to the DP, never a wrong answer).

// the bit planes of one job as 32-bit words: bit j of word k of (pl, ph, pn, pm) = row 32 k + j of the read (its symbol's low / high bit, N, a row
// of the read at all; pn holds no bit past the read's end), bit j of word k of (ql, qh) = text symbol 32 k + j of the window
struct PlaneWords
{
    uint32_t pl[6], ph[6], pn[6], pm[6], ql[7], qh[7];

    __device__ __forceinline__ void set(const uint64_t (&rlo)[3], const uint64_t (&rhi)[3], const uint64_t (&rn)[3],
                                        const uint64_t (&tlo)[4], const uint64_t (&thi)[4], const uint32_t M)
    {
        #pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            pattern_plane_words( k, rlo, rhi, rn, M, pl, ph, pn, pm );
            ql[2*k] = (uint32_t)tlo[k]; ql[2*k+1] = (uint32_t)(tlo[k] >> 32);
            qh[2*k] = (uint32_t)thi[k]; qh[2*k+1] = (uint32_t)(thi[k] >> 32);
        }
        ql[6] = (uint32_t)tlo[3]; qh[6] = (uint32_t)thi[3];
    }
    // mismatch word k (rows 32 k .. 32 k + 31) of the diagonal that lies x <= 31 symbols on in the text planes as they stand (x is wave-uniform
    // wherever this is called: one funnel shift per plane word)
    __device__ __forceinline__ uint32_t mmw(const int k, const uint32_t x) const
    {
        const uint32_t tl = __builtin_amdgcn_alignbit( ql[k + 1], ql[k], x ), th = __builtin_amdgcn_alignbit( qh[k + 1], qh[k], x );
        return (((pl[k] ^ tl) | (ph[k] ^ th)) & pm[k]) | pn[k];
    }
};

// one job of the pass below: scores / sinks as its MODE says, returns the job's flag (what the kernel stores in need_dp[job])
template <int RBITS, int MODE, bool QUAL>
__device__ __forceinline__ uint32_t
ungapped_e2e31_job(const BatchDev& b, const int32_t P, const int32_t G, const int32_t gap_open, const int32_t gap_ext,
                   int32_t* __restrict__ scores, uint2* __restrict__ sinks, const uint32_t job, const int32_t* s_pen,
                   const NarrowRule nr = NarrowRule{ 1, 1, 0u })
{
    constexpr bool LIST = MODE != 0;
    const AlnJob   J = load_job( b, job );
    const uint32_t first = J.first, M = J.M, tb = J.tb, N = scored_text_len( b, J );
    const bool     rev = J.rev, comp = J.comp;

    if (N < M)                                                   // nothing reported (gotoh_banded_inl.h:422-423)
    {
        scores[job] = NVBIO_SCORE_MIN; sinks[job] = make_uint2( 0xFFFFFFFFu, 0xFFFFFFFFu );
        return 0u;
    }
    if (M == 0u || M > 161u) return 1u;                          // planes below hold 192 text symbols

    // bit planes of the read and of the window (bitplanes.h); all loads first, then the bit work
    uint64_t rlo[3], rhi[3], rn[3], tlo[4], thi[4];
    {
        // (the window's planes from the text's, where the batch carries them -- the text as the index build left it, one line per window --,
        // else from its 13 packed words; b.text_planes is wave-uniform)
        ReadWords<RBITS> rw; TextUnits<4> tu;
        load_read_words<RBITS>( b.reads, first, M, rw );
        if (b.text_planes) load_text_units<4,0,3>( b.text_planes, tb, tu );
        else               load_text_words<13>( b.text, tb, N < 192u ? N : 192u, tu );
        read_planes192<RBITS>( rw, first, M, rev, comp, rlo, rhi, rn );
        if (b.text_planes)
        {
            load_text_units<4,3,4>( b.text_planes, tb, tu );     // (see load_text_units: 7 waves per SIMD leave 72 registers)
            text_planes_units<4>( tu, tb, tlo, thi );
        }
        else text_planes_words<13>( tu, tb, tlo, thi );
    }
    const uint32_t mb = M + 30u;
    const uint32_t m  = (mb < N ? mb : N) - (M - 1u);
    // the diagonal loops on 32-bit words: a mismatch word is 5 logic ops, and v_bcnt accumulates the count.  ql0 / qh0: the text planes as
    // loaded (diagonal d = d symbols on: one v_alignbit per word); ql / qh: the chances' copy, moved down one bit per diagonal
    PlaneWords pw;
    pw.set( rlo, rhi, rn, tlo, thi, M );
    const uint32_t (&pl)[6] = pw.pl, (&ph)[6] = pw.ph, (&pn)[6] = pw.pn, (&pm)[6] = pw.pm, (&ql0)[7] = pw.ql, (&qh0)[7] = pw.qh;
    uint32_t ql[7], qh[7];

    uint32_t best_cnt = 0xFFFFFFFFu, best_d = 0;
    int64_t U = 0;
    if (LIST)
    {
        // the first pass left this job's best diagonal and its score in scores / sinks
        U      = scores[job];
        best_d = sinks[job].x - M;
    }
    else
    {
        // A diagonal matters only while its count can still change the outcome: no class of alignments the three chances know settles a job
        // whose best diagonal scores 3 G - P or less (the third chance's `beyond`), so counts above `cap` mean "DP" whatever they are, and
        // without qualities neither does a count above the best one found so far.  The first word of a diagonal (32 rows; about 24
        // mismatches on a diagonal that is not the read's own or its partner across an indel) decides that for the whole wave nearly
        // always: its other words are evaluated only if SOME lane is still interested (a wave-uniform branch) -- 24 of 31 diagonals cost one
        // word instead of six.  The text planes are taken d symbols on with one funnel shift per word (d is a constant of the unrolled loop).
        const int64_t floor_u = 3 * (int64_t)(G < gap_open ? G : gap_open) - P;          // U <= floor_u: DP whatever else holds
        const uint32_t cap = P > 0 ? (uint32_t)((-floor_u - 1) / (int64_t)P) : 0xFFFFFFFEu;   // the largest count with -P cnt > floor_u
        // (the DP's narrow classes: counts up to nr.cnt_max are kept exact too.  This CHANGES A ROUTE: an unclipped job whose best diagonal has
        // more than `cap` mismatches but a U* within class B -- 5 at -6 / -8 / -3 -- used to leave with flag 4 for the gap chance, alone or
        // as a pair member, and now leaves with flag 1 for the DP's class.  For a read with that many substitutions this saves a gap-chance
        // evaluation that could not settle it; the rare indel read whose best diagonal has exactly that count, which the gap chance would
        // have settled, costs a class-B DP instead, and its partner goes to the gap chance alone.  Results are the same either way.)
        const uint32_t cap_x = (!QUAL && nr.cnt_max > cap && N >= M + 30u) ? nr.cnt_max : cap;
        uint32_t cnt_d[QUAL ? 31 : 1];
        #pragma unroll
        for (uint32_t d = 0; d < 31u; ++d)
        {
            const bool on = (d == 0u || d < m);                      // reportable columns are a prefix of 0..30
            uint32_t cnt = (uint32_t)__popc( pw.mmw( 0, d ) );
            const uint32_t thr = QUAL ? cap : (best_cnt < cap_x ? best_cnt : cap_x);
            if (__any( on && cnt <= thr ))
            {
                #pragma unroll
                for (int k = 1; k < 6; ++k) cnt += (uint32_t)__popc( pw.mmw( k, d ) );
            }
            else cnt = 0xFFFFFFFFu;                                  // (partial, and above every lane's threshold)
            if (QUAL) cnt_d[d] = on ? cnt : 0xFFFFFFFFu;
            if (on && cnt <= best_cnt) { best_cnt = cnt; best_d = d; }     // ties: the larger column, as BestSink's `<=`
        }
        if (best_cnt > cap)                                          // (includes: no diagonal evaluated)
        {
            if (!QUAL && best_cnt <= cap_x)
            {
                // out of every chance's reach, but its U* is known and within class B: straight to the DP's narrow role
                const uint32_t cls = narrow_class( nr, -(int64_t)P * (int64_t)best_cnt, best_d, gap_ext );
                if (cls) { scores[job] = -P * (int32_t)best_cnt; sinks[job] = make_uint2( M + best_d, M ); return 1u | (cls << 8); }
            }
            // no diagonal within reach of the three chances: typically a read with an indel.  The gap chance (gap_chance_e2e31_kernel, its own
            // list pass) evaluates the one-gap alignments of such a job exactly; it needs every diagonal inside the text and plain gap terms
            // (not under a quality ramp: see the kernel's header)
            const bool gap_chance = !QUAL && P > 0 && N >= M + 30u && gap_ext < 0 && gap_open <= gap_ext && !(b.algo & NVBIO_ALN_NO_GAP_CHANCE);
            return gap_chance ? 4u : 1u;
        }
        U = -(int64_t)P * (int64_t)best_cnt;
        if (QUAL)
        {
            // no class of alignments the three chances know can be settled below 3 G - P (the third chance's `beyond`): such a job
            // needs the DP whatever its exact U*, so its qualities are not even read
            if (U <= 3 * (int64_t)G - P) return 1u;
            const uint32_t pmax  = (uint32_t)s_pen[63];
            const uint64_t bound = (uint64_t)pmax * best_cnt;                    // a diagonal with P c_d > pmax c_min cannot hold the maximum
            uint32_t cand = 0;
            #pragma unroll
            for (uint32_t d = 0; d < 31u; ++d)
                if (cnt_d[d] != 0xFFFFFFFFu && (uint64_t)(uint32_t)P * cnt_d[d] <= bound) cand |= 1u << d;
            uint32_t best_w = 0xFFFFFFFFu;
            while (cand)                                                          // ascending d: `<=` keeps the larger column on ties
            {
                const uint32_t d = (uint32_t)__builtin_ctz( cand );
                cand &= cand - 1u;
                uint32_t w = 0;
                #pragma unroll
                for (int k = 0; k < 6; ++k)
                {
                    uint32_t mm = pw.mmw( k, d );
                    while (mm)
                    {
                        const uint32_t row = 32u * k + (uint32_t)__builtin_ctz( mm );
                        mm &= mm - 1u;
                        const uint32_t qq = b.quals[rev ? first + M - 1u - row : first + row];
                        w += (uint32_t)s_pen[qq < 63u ? qq : 63u];
                    }
                }
                if (w <= best_w) { best_w = w; best_d = d; }
            }
            U = -(int64_t)best_w;
        }
    }
    bool settled = U > (int64_t)G;
    auto stash = [&]() { scores[job] = (int32_t)U; sinks[job] = make_uint2( M + best_d, M ); };
    const bool second_applies = !settled && (int64_t)G - P < U && 2 * (int64_t)G < U && N >= M + 30u && !(b.algo & NVBIO_ALN_NO_SECOND_CHANCE);
    if (MODE == 0 && second_applies)
    {
        int32_t gmax = 0;
        while (gmax < 5 && (int64_t)gap_open + (int64_t)gmax * gap_ext >= U) ++gmax;
        if (gmax >= 1 && gmax <= 4) { stash(); return 3u; }                     // for the second-chance launch
    }
    if (MODE == 1 && second_applies)
    {
        // Second chance (two mismatches at nvBowtie's -6 / -8 / -3).  U* <= G, but one gap plus one mismatch and two gaps
        // both score below U*: the only gapped alignments that could reach U* have exactly ONE gap and NO mismatch, i.e. a
        // prefix of the read matching one diagonal exactly and the rest matching a diagonal g columns away, for the few gap
        // lengths g with open + (g-1) ext >= U*.  With lead_d / tail_d = the exactly matching prefix / suffix lengths of
        // diagonal d, a text gap (d-g -> d) exists iff lead_{d-g} + tail_d >= M, a pattern gap (d -> d-g) iff
        // lead_d + tail_{d-g} + g >= M.  If none exists the optimum is U* and only ungapped diagonals reach it.
        // (N >= M + 30: all 31 diagonals lie inside the text, so no sentinel cell is involved.)
        int32_t gmax = 0;
        while (gmax < 5 && (int64_t)gap_open + (int64_t)gmax * gap_ext >= U) ++gmax;      // lengths 1..gmax can reach U*
        if (gmax >= 1 && gmax <= 4)
        {
            #pragma unroll
            for (int k = 0; k < 7; ++k) { ql[k] = ql0[k]; qh[k] = qh0[k]; }
            uint32_t lead_prev[4] = { 0, 0, 0, 0 }, tail_prev[4] = { 0, 0, 0, 0 };        // diagonals d-1 .. d-4
            bool gapped = false;
            for (uint32_t d = 0; d < 31u && !gapped; ++d)
            {
                // first / last mismatching row of the diagonal, searched from the two ends and only as far as needed: on a diagonal that
                // is not (nearly) the read's own, word 0 and the top word already hold mismatches, and a word is evaluated by the wave
                // only while some lane is still looking -- 3 word evaluations per diagonal instead of 12 (the values are the same)
                uint32_t first = M, last = 0xFFFFFFFFu;
                #pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (first == M)
                    {
                        const uint32_t mm = (((pl[k] ^ ql[k]) | (ph[k] ^ qh[k])) & pm[k]) | pn[k];
                        if (mm) first = 32u * k + (uint32_t)__builtin_ctz( mm );
                    }
                #pragma unroll
                for (int k = 5; k >= 0; --k)
                    if (last == 0xFFFFFFFFu)
                    {
                        const uint32_t mm = (((pl[k] ^ ql[k]) | (ph[k] ^ qh[k])) & pm[k]) | pn[k];
                        if (mm) last = 32u * k + 31u - (uint32_t)__builtin_clz( mm );
                    }
                const uint32_t lead = first;                                               // rows 0..lead-1 match
                const uint32_t tail = (last == 0xFFFFFFFFu) ? M : M - 1u - last;           // the last `tail` rows match
                #pragma unroll
                for (int g = 1; g <= 4; ++g)
                    if (g <= gmax && d >= (uint32_t)g)
                    {
                        if (lead_prev[g - 1] + tail >= M) gapped = true;                   // text gap of g: diagonal d-g, then d
                        if (lead + tail_prev[g - 1] + (uint32_t)g >= M) gapped = true;     // pattern gap of g: diagonal d, then d-g
                    }
                #pragma unroll
                for (int k = 3; k > 0; --k) { lead_prev[k] = lead_prev[k - 1]; tail_prev[k] = tail_prev[k - 1]; }
                lead_prev[0] = lead; tail_prev[0] = tail;
                #pragma unroll
                for (int k = 0; k < 6; ++k)
                {
                    ql[k] = __builtin_amdgcn_alignbit( ql[k + 1], ql[k], 1u );
                    qh[k] = __builtin_amdgcn_alignbit( qh[k + 1], qh[k], 1u );
                }
                ql[6] >>= 1; qh[6] >>= 1;
            }
            settled = !gapped;
        }
    }
    // which classes of gapped alignments can reach U* by score alone (third chance; two or three mismatches at -6 / -8 / -3):
    //   A  one gap of g <= gmax0 symbols, no mismatch          (open + (g-1) ext >= U*)
    //   B  one gap of g <= gmax1 symbols and ONE mismatch      (open + (g-1) ext - P >= U*)
    //   C  two gaps of one symbol each, no mismatch            (2 open >= U*)
    // anything beyond (one gap + two mismatches, two gaps with a longer one or a mismatch, three gaps, gaps over 4) means DP.
    const int64_t go = gap_open, ge = gap_ext;
    int32_t gmax0 = 0, gmax1 = 0;
    while (gmax0 < 5 && go + (int64_t)gmax0 * ge >= U) ++gmax0;
    while (gmax1 < 5 && go + (int64_t)gmax1 * ge - P >= U) ++gmax1;
    const bool two11  = 2 * go >= U;
    const bool beyond = gmax0 > 4 || gmax1 > 4 || go - 2 * (int64_t)P >= U || 2 * go + ge >= U || 2 * go - P >= U || 3 * go >= U || ge < go;
    const bool third_applies = !settled && N >= M + 30u && !beyond && gmax0 >= 1 && (gmax1 >= 1 || two11);
    if (MODE == 0 && third_applies)
    {
        stash();                                                 // for the third-chance launch
        return 2u;
    }
    if (MODE != 0 && third_applies)                              // (MODE 1: a job the second chance did not settle)
    {
        // With lead0/lead1(d) = rows before the first / second mismatch of diagonal d and tail0/tail1(d) = rows after its last /
        // last-but-one mismatch:
        //   text gap g (prefix on d-g, suffix on d) with <= e mismatches  iff  lead_i(d-g) + tail_{e-i}(d) >= M for some i <= e
        //   pattern gap g (prefix on d, suffix on d-g)                    iff  lead_i(d) + tail_{e-i}(d-g) + g >= M
        //   C through a middle diagonal b with neighbours a, c = b +- 1: the prefix on a may run to row lo = lead0(a) (+1 after a
        //     pattern gap), the suffix on c may start at row hi = M - tail0(c) (-1 before a pattern gap): it exists iff lo >= hi
        //     or b has no mismatch in rows [lo, hi).
        // Existence is over-approximated (band limits and reportable columns are ignored), which only costs a DP.  If no class
        // has a member the optimum is U* and only ungapped diagonals reach it.  A gapped alignment that merely TIES U* also goes
        // to the DP (the sink rule decides there).  (N >= M + 30: all 31 diagonals lie inside the text, no sentinel cell.)
        #pragma unroll
        for (int k = 0; k < 7; ++k) { ql[k] = ql0[k]; qh[k] = qh0[k]; }
        uint32_t lead0_p[4] = { 0, 0, 0, 0 }, lead1_p[4] = { 0, 0, 0, 0 }, tail0_p[4] = { 0, 0, 0, 0 }, tail1_p[4] = { 0, 0, 0, 0 };   // d-1 .. d-4
        bool gapped = false;
        uint32_t mwp[6] = { 0, 0, 0, 0, 0, 0 };
        for (uint32_t d = 0; d <= 31u && !gapped; ++d)
        {
            const bool have = d < 31u;                                                  // d = 31 only closes class C for b = 30
            // the first two and the last two mismatching rows of the diagonal, searched from the two ends and only as far as needed: on a
            // diagonal that is not (nearly) the read's own the first and the top word already hold two mismatches each, and a word is
            // evaluated by the wave only while some lane is still looking (the values are the same as with all 12 word evaluations)
            uint32_t first = M, second = M, last = 0xFFFFFFFFu, last2 = 0xFFFFFFFFu;
            #pragma unroll
            for (int k = 0; k < 6; ++k)
                if (have && __any( second == M ))                       // a wave-uniform branch: really skipped when no lane is looking
                {
                    uint32_t w = (second == M) ? ((((pl[k] ^ ql[k]) | (ph[k] ^ qh[k])) & pm[k]) | pn[k]) : 0u;
                    if (first == M && w) { first = 32u * k + (uint32_t)__builtin_ctz( w ); w &= w - 1u; }
                    if (first != M && second == M && w) second = 32u * k + (uint32_t)__builtin_ctz( w );
                }
            #pragma unroll
            for (int k = 5; k >= 0; --k)
                if (have && __any( last2 == 0xFFFFFFFFu ))
                {
                    uint32_t w = (last2 == 0xFFFFFFFFu) ? ((((pl[k] ^ ql[k]) | (ph[k] ^ qh[k])) & pm[k]) | pn[k]) : 0u;
                    if (last == 0xFFFFFFFFu && w) { const uint32_t t = 31u - (uint32_t)__builtin_clz( w ); last = 32u * k + t; w &= ~(1u << t); }
                    if (last != 0xFFFFFFFFu && last2 == 0xFFFFFFFFu && w) last2 = 32u * k + 31u - (uint32_t)__builtin_clz( w );
                }
            const uint32_t lead0 = first, lead1 = second;                               // rows before the 1st / 2nd mismatch
            const uint32_t tail0 = (last  == 0xFFFFFFFFu) ? M : M - 1u - last;          // rows after the last / last-but-one
            const uint32_t tail1 = (last2 == 0xFFFFFFFFu) ? M : M - 1u - last2;
            if (have)
            {
                #pragma unroll
                for (int g = 1; g <= 4; ++g)
                    if (d >= (uint32_t)g)
                    {
                        if (g <= gmax0)
                        {
                            if (lead0_p[g - 1] + tail0 >= M) gapped = true;                                   // A, text gap
                            if (lead0 + tail0_p[g - 1] + (uint32_t)g >= M) gapped = true;                     // A, pattern gap
                        }
                        if (g <= gmax1)
                        {
                            if (lead0_p[g - 1] + tail1 >= M || lead1_p[g - 1] + tail0 >= M) gapped = true;    // B, text gap
                            if (lead0 + tail1_p[g - 1] + (uint32_t)g >= M || lead1 + tail0_p[g - 1] + (uint32_t)g >= M) gapped = true;
                        }
                    }
            }
            if (two11 && d >= 1u)
            {
                // middle diagonal b = d-1 (words mmp); neighbours d-2 (lead0_p[1] / tail0_p[1], if d >= 2) and d (if have)
                int32_t lo_c[2], hi_c[2]; int n_lo = 0, n_hi = 0;
                if (d >= 2u) { lo_c[n_lo++] = (int32_t)lead0_p[1];        hi_c[n_hi++] = (int32_t)M - (int32_t)tail0_p[1] - 1; }   // a = b-1: text gap in; c = b-1: pattern gap out
                if (have)    { lo_c[n_lo++] = (int32_t)lead0 + 1;         hi_c[n_hi++] = (int32_t)M - (int32_t)tail0; }           // a = b+1: pattern gap in; c = b+1: text gap out
                for (int x = 0; x < n_lo; ++x)
                    for (int y = 0; y < n_hi; ++y)
                    {
                        const int32_t lo = lo_c[x], hi = hi_c[y];
                        if (lo >= hi) { gapped = true; continue; }
                        // cheap first: b's first or last mismatch inside [lo, hi) settles it (nearly always, b being an unrelated
                        // diagonal); only otherwise look at the words
                        const int32_t bf = (int32_t)lead0_p[0], bl = (int32_t)M - 1 - (int32_t)tail0_p[0];
                        bool any = (bf >= lo && bf < hi) || (tail0_p[0] < M && bl >= lo && bl < hi);
                        bool full = !any;
                        if (__any( !any ))
                        {
                            // next: the 32 rows from lo on (two of b's words, picked by lo's word index) -- on an unrelated diagonal they hold a
                            // mismatch, which settles it; only an interval that is longer AND clean so far walks all the words
                            const uint32_t wi = (uint32_t)lo >> 5;
                            uint32_t w_lo = mwp[0], w_hi = mwp[1];
                            #pragma unroll
                            for (int k = 1; k < 6; ++k)
                            {
                                const uint32_t next = k < 5 ? mwp[k < 5 ? k + 1 : 5] : 0u;
                                w_lo = wi == (uint32_t)k ? mwp[k] : w_lo;
                                w_hi = wi == (uint32_t)k ? next   : w_hi;
                            }
                            uint32_t rows32 = __builtin_amdgcn_alignbit( w_hi, w_lo, (uint32_t)lo & 31u );      // b's mismatches in rows lo .. lo + 31
                            const int32_t span = hi - lo;                                                        // > 0 here
                            if (span < 32) rows32 &= (1u << span) - 1u;
                            if (!any && wi < 6u) { if (rows32) { any = true; full = false; } else if (span <= 32) full = false; }
                        }
                        if (full)
                        {
                            #pragma unroll
                            for (int k = 0; k < 6; ++k)
                            {
                                const int32_t a0 = lo - 32 * k > 0 ? lo - 32 * k : 0, a1 = hi - 32 * k < 32 ? hi - 32 * k : 32;
                                if (a0 < a1)
                                {
                                    const uint32_t hi_m = (a1 >= 32) ? 0xFFFFFFFFu : ((1u << a1) - 1u);
                                    const uint32_t lo_m = (1u << a0) - 1u;                                       // a0 < a1 <= 32 -> a0 <= 31
                                    // word k of the middle diagonal d-1: kept from the previous iteration
                                    any = any || ((mwp[k] & hi_m & ~lo_m) != 0u);
                                }
                            }
                        }
                        if (!any) gapped = true;
                    }
            }
            #pragma unroll
            for (int k = 3; k > 0; --k) { lead0_p[k] = lead0_p[k - 1]; lead1_p[k] = lead1_p[k - 1]; tail0_p[k] = tail0_p[k - 1]; tail1_p[k] = tail1_p[k - 1]; }
            lead0_p[0] = lead0; lead1_p[0] = lead1; tail0_p[0] = tail0; tail1_p[0] = tail1;
            if (two11 && have)                                   // this diagonal's mismatch words: the middle diagonal of the next iteration
            {
                #pragma unroll
                for (int k = 0; k < 6; ++k) mwp[k] = (((pl[k] ^ ql[k]) | (ph[k] ^ qh[k])) & pm[k]) | pn[k];
            }
            #pragma unroll
            for (int k = 0; k < 6; ++k)
            {
                ql[k] = __builtin_amdgcn_alignbit( ql[k + 1], ql[k], 1u );
                qh[k] = __builtin_amdgcn_alignbit( qh[k + 1], qh[k], 1u );
            }
            ql[6] >>= 1; qh[6] >>= 1;
        }
        settled = !gapped;
    }
    if (settled)
    {
        scores[job] = (int32_t)U; sinks[job] = make_uint2( M + best_d, M );
        return 0u;
    }
    if (MODE == 0 && !QUAL && N >= M + 30u)
    {
        const uint32_t cls = narrow_class( nr, U, best_d, gap_ext );
        if (cls) { stash(); return 1u | (cls << 8); }
    }
    return 1u;
}

} // namespace nvbio_amd
