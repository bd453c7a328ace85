// band31_packed.hip -- the packed band-31 Gotoh DP for gfx950: two alignments per lane in 16-bit halves (int16 or binary16), over every job
// of a batch or over the job lists the end-to-end shortcuts leave (band31_stage.hip, gotoh_full.hip).
#include "band31_jobs.h"
#include "pk_lanes.h"

namespace nvbio_amd {

// ---------------------------------------------------------------------------------------------
// 16-bit packed variant for the production case (band 31, any alignment type): one lane owns TWO
// alignments, one in each half of every register, so H[31]/F[31] of both take the registers one
// alignment took before and every add / max is a v_pk_*_i16 doing two cells.  Exactness conditions,
// checked on the host (packed_ok; else the int32 kernel runs): LOCAL scores fit 10 bits
// (match * max_read_len <= 1000, so that (score << 5 | column) fits an int16), GLOBAL / SEMI_GLOBAL
// scores stay within +-8000 ((max_read_len + 32) * largest step), and penalties are < 4096, so that
// the -16384 stand-in for the reference's infimum can never win a max against a real score nor
// wrap.  The row-0 / column-30 infimum cells behave exactly as in the int32 kernel.  With a job
// list (the jobs the ungapped shortcut could not settle) lane p works on list entries 2p, 2p+1.
// ---------------------------------------------------------------------------------------------

// 32 bits of a big-endian packed stream starting at absolute bit position `bit`, assembled from the
// two words (a = word bit>>5, b = the next one) that were loaded one chunk earlier
__device__ __forceinline__ uint32_t funnel32(const uint32_t a, const uint32_t b, const uint32_t bit)
{
    const uint32_t sh = bit & 31u;
    return sh ? ((a << sh) | (b >> (32u - sh))) : a;
}
__device__ __forceinline__ uint32_t clamp_u32(const int64_t v, const uint32_t lo, const uint32_t hi)
{
    return v < (int64_t)lo ? lo : (v > (int64_t)hi ? hi : (uint32_t)v);
}

// bit k of the result = bit 2k of x
__device__ __forceinline__ uint32_t even_bits64(uint64_t x)
{
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16));
    return (uint32_t)x;
}

// Rows are processed in chunks of 8.  At the top of a chunk every lane assembles the chunk's 8 read
// symbols and 8 incoming text symbols (per alignment) from words loaded one chunk EARLIER, then
// issues the loads for the next chunk: one wave-uniform wait point per 8 rows with an 8-row
// (~5,000 instruction) head start, and no per-row branches.  Reads are packed RBITS (2 or 4) per
// symbol, the text 2 bits per symbol.
// MINW: the occupancy the register allocator must reach.  3 waves per SIMD leave 168 VGPRs: about 90 registers of prologue / epilogue
// state spill (the scratch accesses sit outside the row loop).  2 waves leave 256: nothing spills.  Which is faster is measured, not
// assumed: 3 waves won while the row loop still had idle issue slots to fill; with the hand-ordered loop 2 waves are 4 % ahead and
// are the default, NVBIO_ALN_PK_THREE_WAVES runs the other build.
// RAGGED (GLOBAL / SEMI_GLOBAL; NVBIO_ALN_RAGGED_READS): a lane whose two alignments differ in length still takes ONE pass: the shorter one
// starts late, at row pad = (rows of the longer) - (its own rows), so that both end in the same row and report from the band there.  Its
// streams are read at row - pad (before its start it computes on whatever they hold), and in the row it starts its half of the band and of
// the text cache is set to the initial state -- one extra wave-level branch per row while some lane of the wave is still waiting to start.
// FP (M0, not LOCAL; the host checks that every score stays inside +-2040): the two lanes of a register are binary16 numbers.  Integers of that
// size, their sums and maxima are exact there, the mismatch flag becomes 2^-7 (bit 13 of each half) against a penalty scaled by 128 in one
// v_pk_fma_f16, and h = max( f, d, E ) is ONE v_pk_maximum3_f16: 9 operations per cell instead of 10.  (The -16384 stand-in for the reference's
// infimum stays where it is under + GE: 16 is the spacing of binary16 there.)
// NARROW (the binary16 SEMI_GLOBAL build only; NVBIO_ALN_NO_NARROW_DP runs the build without it): ONE launch over three job lists.  The first pass
// gives a job that leaves for the DP with a known best diagonal score L = U* (stashed in scores[job]) a class by L alone: with match = 0 every step
// of a path scores <= 0, so every cell on a path holds H >= the path's final score; L is achievable, so the optimum is >= L and a cell with H < L
// lies on no optimal path.  Standing delta columns off the best diagonal costs open + (delta - 1) ext, so for a window centred on that diagonal
// (column 15) everything beyond +-r(L) of it is dead once the free-start paths of row 0 have died: class A = columns 9..21 (w <= 6), class B =
// columns 7..23 (w <= 8).  A workgroup has one role, taken from blockIdx.x: the full list's workgroups come first, then class B's, then class A's
// (the shortest jobs fill the tail).  A narrow job runs
//   1. rows 0 .. NARROW_FULL_ROWS - 1 with the full row body;
//   2. at row NARROW_FULL_ROWS the qualification, per half of the lane: every outer H and F must be < L; the outer H / Hg / F then become the
//      infimum (so the report loop at the end needs no change);
//   3. the remaining rows with the row body over columns LO..HI (column LO takes no E, column HI no F) and a monitor: the running maximum of
//      what flows from the inner columns into the outer ones -- max( Hg[LO], F[LO] + ext ) of the row before into column LO - 1, and
//      E' = max( hg, E + ext ) of column HI into column HI + 1;
//   4. a half that qualified and whose monitor stayed < L reports as the full band does; any other half reports nothing, keeps its stash in
//      scores[] and puts its job on the redo list, over which the build without NARROW runs behind this launch.
// Exactness, by induction over the rows from NARROW_FULL_ROWS on: every input of an outer cell is another outer cell or one of the monitored
// flows, hence < L; all steps are <= 0; so every outer cell is < L.  An inner cell's narrow value is its true value unless both are < L (a path
// that gives a cell a value >= L runs through cells >= L only: inner ones from row NARROW_FULL_ROWS on, exactly computed ones before).  The
// optimum is >= L, so it sits in an inner cell of the last row with its true value, and no outer cell can tie it.  L is only a lower bound: a
// gapped optimum above U* is found like any other.
constexpr uint32_t NARROW_FULL_ROWS = 24u;                       // three chunks of 8 rows (simulated: no outer column alive at row 24, some at row 16)

template <int TYPE, int RBITS, int MINW = 3, bool M0 = false, bool RAGGED = false, bool FP = false, bool NARROW = false>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(MINW, 3)))
banded_gotoh_band31_pk_kernel(const BatchDev b, const SchemeDev sc, int32_t* __restrict__ scores, uint2* __restrict__ sinks,
                              const uint32_t* __restrict__ job_list, const uint32_t* __restrict__ job_count, const NarrowJobs nj)
{
    constexpr int BAND = 31;
    constexpr uint32_t RMASK = (1u << RBITS) - 1u;
    static_assert( !FP || (M0 && TYPE != NVBIO_LOCAL), "the binary16 build: match = 0, GLOBAL / SEMI_GLOBAL" );
    static_assert( !NARROW || (FP && !RAGGED && TYPE == NVBIO_SEMI_GLOBAL), "the narrow roles: the binary16 SEMI_GLOBAL build, equal read lengths" );
    typedef typename PkLanes<FP>::type v2;
    __shared__ int32_t s_mm[64];
    fill_mismatch_table( s_mm, sc );

    // with a job list (the jobs the ungapped pass could not settle) lane p works on entries 2p and 2p+1 of the list
    uint32_t n_jobs = job_list ? *job_count : b.n;
    uint32_t group = blockIdx.x;
    int role = 0;                                                    // 0: the full band, 1: class B, 2: class A (uniform over the workgroup)
    if (NARROW)
    {
        const uint32_t nb_full = (n_jobs + 255u) / 256u, n_b = *nj.count_b, nb_b = (n_b + 255u) / 256u;
        if (group >= nb_full)
        {
            group -= nb_full; role = 1; job_list = nj.list_b; n_jobs = n_b;
            if (group >= nb_b) { group -= nb_b; role = 2; job_list = nj.list_a; n_jobs = *nj.count_a; }
        }
    }
    const uint32_t pair = group * blockDim.x + threadIdx.x;
    if (2u * pair >= n_jobs) return;
    const uint32_t* __restrict__ rwords = (const uint32_t*)b.reads;
    const uint32_t* __restrict__ twords = (const uint32_t*)b.text;

    uint32_t first[2], M[2], tb[2], N[2], rows_all[2], out_id[2];
    bool     rev[2], comp[2], valid[2];
    #pragma unroll
    for (int u = 0; u < 2; ++u)
    {
        const uint32_t slot = 2u * pair + u;
        valid[u] = slot < n_jobs;
        const uint32_t ss  = valid[u] ? slot : 2u * pair;
        const uint32_t jj  = job_list ? job_list[ss] : ss;
        out_id[u] = jj;
        const AlnJob J = load_job( b, jj );
        first[u] = J.first; M[u] = J.M; rev[u] = J.rev; comp[u] = J.comp; tb[u] = J.tb;
        N[u]     = scored_text_len( b, J );
        // rows this alignment really computes: none when the text is shorter than the pattern (nothing reported)
        rows_all[u] = (valid[u] && N[u] >= M[u]) ? M[u] : 0u;
    }

    // word ranges a stream may touch (loads are clamped into them; symbols outside are never used)
    uint32_t r_lo[2], r_hi[2], t_lo[2], t_hi[2];
    #pragma unroll
    for (int u = 0; u < 2; ++u)
    {
        r_lo[u] = (uint32_t)(((uint64_t)first[u] * RBITS) >> 5);
        r_hi[u] = (uint32_t)(((uint64_t)(first[u] + (M[u] ? M[u] - 1u : 0u)) * RBITS) >> 5);
        t_lo[u] = tb[u] >> 4;
        t_hi[u] = (tb[u] + (N[u] ? N[u] - 1u : 0u)) >> 4;
    }

    // storage position (symbol index) where the read chunk of rows [r0, r0+8) starts: forward reads start
    // at first+r0 and walk up; reversed reads cover [first+M-1-r0-7, first+M-1-r0] and walk down from its top
    auto read_chunk_start = [&](const int u, const uint32_t r0) -> int64_t {
        return rev[u] ? (int64_t)first[u] + (int64_t)M[u] - 1 - (int64_t)r0 - 7 : (int64_t)first[u] + r0;
    };
    auto read_chunk_start_at = [&](const int u, const int64_t r0) -> int64_t {      // RAGGED: rows before the alignment's start are negative
        return rev[u] ? (int64_t)first[u] + (int64_t)M[u] - 1 - r0 - 7 : (int64_t)first[u] + r0;
    };

    const uint32_t qadj = (uint32_t)((uintptr_t)b.quals & 3u);      // the quality stream need not be 4-byte aligned
    const uint32_t* __restrict__ qwords = (const uint32_t*)((uintptr_t)b.quals - qadj);
    const bool has_quals = !NARROW && (b.quals != nullptr);         // (classes are formed only for batches without qualities)

    const v2 GO = pk_of<v2>( sc.pat_go, sc.pat_go ), GE = pk_of<v2>( sc.pat_ge, sc.pat_ge );
    const v2 INF = pk_of<v2>( -16384, -16384 ), ZERO = pk_of<v2>( 0, 0 );
    const v2s K32 = pk( 32, 32 );
    const int V = sc.match;
    const int S_noq = s_mm[0];                                       // without qualities every row scores a mismatch like this
    uint32_t cx[2], lim[2];
    #pragma unroll
    for (int u = 0; u < 2; ++u)
    {
        cx[u]  = comp[u] ? 3u : 0u;                                  // complement: A<->T, C<->G
        lim[u] = N[u] > (uint32_t)(BAND - 1) ? N[u] - (uint32_t)(BAND - 1) : 0u;     // row i's column 30 lies past the text end iff i >= lim
    }

    int32_t  best[2]   = { NVBIO_SCORE_MIN, NVBIO_SCORE_MIN };
    uint32_t best_x[2] = { 0xFFFFFFFFu, 0xFFFFFFFFu }, best_y[2] = { 0xFFFFFFFFu, 0xFFFFFFFFu };
    // the narrow roles: the largest value seen so far that must stay below L -- the outer cells at the qualification, then the monitored flows
    v2 mon = INF;

    // GLOBAL / SEMI_GLOBAL report from the band after an alignment's LAST row (:624-645).  To keep that out
    // of the row loop, a lane whose two alignments have different lengths runs them one after the other
    // (two passes, one half active each); equal lengths -- the normal case for a read batch -- take one pass.
    // LOCAL reports every cell as it goes and always takes one pass.
    const bool want0 = valid[0] && N[0] >= M[0], want1 = valid[1] && N[1] >= M[1];
    const bool split = (TYPE != NVBIO_LOCAL) && !RAGGED && want0 && want1 && M[0] != M[1];
    // RAGGED: rows the shorter alignment waits before it starts
    const uint32_t rows_max = rows_all[0] > rows_all[1] ? rows_all[0] : rows_all[1];
    uint32_t pad[2] = { 0u, 0u };
    if (RAGGED && TYPE != NVBIO_LOCAL) { pad[0] = rows_max - rows_all[0]; pad[1] = rows_max - rows_all[1]; }

    // (one copy of the passes per role: the roles' row bodies then share no registers for their loop invariants -- written as one loop with
    // the role tested per chunk, the build spilled 64 registers)
    auto run_passes = [&](auto ROLE_)
    {
    constexpr int ROLE = decltype(ROLE_)::value;
    for (int pass = 0; pass < (split ? 2 : 1); ++pass)
    {
        uint32_t rows_u[2];
        rows_u[0] = (split && pass != 0) ? 0u : rows_all[0];
        rows_u[1] = (split && pass != 1) ? 0u : rows_all[1];
        const uint32_t rows = rows_u[0] > rows_u[1] ? rows_u[0] : rows_u[1];

        // ---- text cache: two bit planes per alignment, c0 / c1 = low / high bits of the symbols.  Inside a row column j sits at bit
        // 30-j: the row's incoming symbol (column 30) is shifted in at bit 0 (one v_alignbit per plane) and every other column
        // thereby moves to the next row's position; between rows the planes hold columns 0..29 at bits 29-j ------------------------
        uint32_t c0[2], c1[2], c0i[2] = { 0, 0 }, c1i[2] = { 0, 0 };
        #pragma unroll
        for (int u = 0; u < 2; ++u)
        {
            const uint32_t w  = tb[u] >> 4;
            const uint32_t w0 = twords[clamp_u32( w,      t_lo[u], t_hi[u] )];
            const uint32_t w1 = twords[clamp_u32( w + 1u, t_lo[u], t_hi[u] )];
            const uint32_t w2 = twords[clamp_u32( w + 2u, t_lo[u], t_hi[u] )];
            const uint32_t bit = (tb[u] & 15u) * 2u;
            const uint64_t hi = ((uint64_t)funnel32( w0, w1, bit ) << 32) | funnel32( w1, w2, bit );
            uint64_t c = hi & ~0xFull;                               // 30 symbols = top 60 bits, column j at bits [62-2j, 63-2j]
            // symbols at or past the text end read as 3 (the 255 sentinel through a 2-bit cache)
            if (N[u] < 30u) c |= (~0ull >> (2u * N[u])) & ~0xFull;
            // even / odd bits of c, gathered: column j at bit 31-j, moved to bit 29-j (the row's incoming symbol is shifted in at bit 0)
            c0[u] = even_bits64( c ) >> 2;
            c1[u] = even_bits64( c >> 1 ) >> 2;
            if (RAGGED) { c0i[u] = c0[u]; c1i[u] = c1[u]; }
        }

        // ---- stream words for chunk 0 (loaded now, consumed at the top of the loop) ----------------------
        uint32_t ra[2], rb[2], ta[2], tbw[2];
        uint32_t qa[2] = { 0, 0 }, qb[2] = { 0, 0 }, qc[2] = { 0, 0 };  // quality bytes: 3 words cover 8 unaligned bytes
        auto issue_loads = [&](const uint32_t r0) {
            if (has_quals)
            {
                #pragma unroll
                for (int u = 0; u < 2; ++u)
                {
                    const int64_t qw  = ((RAGGED ? read_chunk_start_at( u, (int64_t)r0 - pad[u] ) : read_chunk_start( u, r0 )) + qadj) >> 2;        // byte position / 4
                    const uint32_t lo = (first[u] + qadj) >> 2, hi = (first[u] + qadj + (M[u] ? M[u] - 1u : 0u)) >> 2;
                    qa[u] = qwords[clamp_u32( qw,     lo, hi )];
                    qb[u] = qwords[clamp_u32( qw + 1, lo, hi )];
                    qc[u] = qwords[clamp_u32( qw + 2, lo, hi )];
                }
            }
            #pragma unroll
            for (int u = 0; u < 2; ++u)
            {
                const int64_t  rbit = (RAGGED ? read_chunk_start_at( u, (int64_t)r0 - pad[u] ) : read_chunk_start( u, r0 )) * RBITS;
                const int64_t  rw   = rbit >> 5;                          // arithmetic shift: floor for negatives
                ra[u]  = rwords[clamp_u32( rw,     r_lo[u], r_hi[u] )];
                rb[u]  = rwords[clamp_u32( rw + 1, r_lo[u], r_hi[u] )];
                // text symbol entering column 30 at row r0 (RAGGED: of the alignment's own row r0 - pad, possibly before the window)
                const int64_t  tw   = RAGGED ? (((int64_t)tb[u] + (int64_t)r0 - pad[u] + (BAND - 1)) >> 4)
                                             : (int64_t)(((uint64_t)tb[u] + r0 + (BAND - 1)) >> 4);
                ta[u]  = twords[clamp_u32( tw,     t_lo[u], t_hi[u] )];
                tbw[u] = twords[clamp_u32( tw + 1, t_lo[u], t_hi[u] )];
            }
        };
        issue_loads( 0 );

        v2 H[BAND], Hg[BAND], F[BAND];                               // Hg = H + GO, kept beside H: feeds the next row's F and this row's E
        #pragma unroll
        for (int j = 0; j < BAND; ++j)
        {
            const int h0 = (TYPE == NVBIO_GLOBAL && j > 0) ? sc.txt_go + (j - 1) * sc.txt_ge : 0;      // init_row_zero (:37-68)
            H[j] = pk_of<v2>( h0, h0 ); F[j] = INF; Hg[j] = H[j] + GO;
        }

        // one chunk of 8 rows over columns LO..HI of the band
        auto do_chunk = [&](const uint32_t r0, auto LO_, auto HI_)
        {
            // ---- assemble this chunk from the words loaded a chunk ago, then request the next chunk ----
            uint32_t rchunk[2], tchunk[2], tchunk1[2]; int rsh[2], rstep[2];
            uint64_t qchunk[2] = { 0, 0 }; int qsh[2], qstep[2];
            #pragma unroll
            for (int u = 0; u < 2; ++u)
            {
                if (has_quals)
                {
                    // 8 quality bytes of the chunk, byte k of the chunk at bits [8k, 8k+7] (memory order)
                    const uint32_t bs = ((uint32_t)(((RAGGED ? read_chunk_start_at( u, (int64_t)r0 - pad[u] ) : read_chunk_start( u, r0 )) + qadj) & 3)) * 8u;
                    const uint32_t lo = bs ? ((qa[u] >> bs) | (qb[u] << (32u - bs))) : qa[u];
                    const uint32_t hi = bs ? ((qb[u] >> bs) | (qc[u] << (32u - bs))) : qb[u];
                    qchunk[u] = ((uint64_t)hi << 32) | lo;
                }
                qsh[u] = rev[u] ? 56 : 0; qstep[u] = rev[u] ? -8 : 8;
                const int64_t rbit = (RAGGED ? read_chunk_start_at( u, (int64_t)r0 - pad[u] ) : read_chunk_start( u, r0 )) * RBITS;
                rchunk[u] = funnel32( ra[u], rb[u], (uint32_t)(rbit & 31) );
                rsh[u]    = rev[u] ? (32 - RBITS) - 7 * RBITS : (32 - RBITS);   // row 0 of the chunk: last / first symbol
                rstep[u]  = rev[u] ? RBITS : -RBITS;
                const uint32_t tsym = RAGGED ? (uint32_t)(((int64_t)tb[u] + (int64_t)r0 - pad[u] + (BAND - 1)) & 15)
                                             : (uint32_t)(((uint64_t)tb[u] + r0 + (BAND - 1)) & 15u);
                uint32_t tc = funnel32( ta[u], tbw[u], tsym * 2u );
                // symbols at or past the text end enter the cache as 3 (the 255 sentinel through a 2-bit cache): symbol k of the
                // chunk is text symbol r0 + 30 + k
                const int64_t kk = RAGGED ? (int64_t)N[u] - (int64_t)(BAND - 1) - ((int64_t)r0 - pad[u]) : (int64_t)N[u] - (int64_t)(BAND - 1) - (int64_t)r0;
                if (kk < 16) tc |= (kk <= 0) ? 0xFFFFFFFFu : (0xFFFFFFFFu >> (2u * (uint32_t)kk));
                tchunk[u]  = tc;                                     // top bit = high bit of the next symbol
                tchunk1[u] = tc << 1;                                // top bit = its low bit
            }
            if (r0 + 8u < rows) issue_loads( r0 + 8u );

            const uint32_t r_end = (r0 + 8u < rows) ? 8u : rows - r0;
            // the chunk's rows over columns LO..HI of the band (0..30: the whole band)
            auto chunk_rows = [&](auto LO_, auto HI_)
            {
            constexpr int LO = decltype(LO_)::value, HI = decltype(HI_)::value;
            for (uint32_t t = 0; t < r_end; ++t)
            {
                const uint32_t i = r0 + t;
                if (RAGGED && TYPE != NVBIO_LOCAL)
                {
                    // an alignment that starts in this row: its half of the band and of the text cache to the initial state
                    const bool s0 = pad[0] != 0u && i == pad[0], s1 = pad[1] != 0u && i == pad[1];
                    if (s0 || s1)
                    {
                        #pragma unroll
                        for (int j = 0; j < BAND; ++j)
                        {
                            const int h0 = (TYPE == NVBIO_GLOBAL && j > 0) ? sc.txt_go + (j - 1) * sc.txt_ge : 0;
                            const v2 hh = pk_of<v2>( h0, h0 ), hhg = pk_of<v2>( h0 + sc.pat_go, h0 + sc.pat_go );
                            if (s0) { H[j].x = hh.x; F[j].x = INF.x; Hg[j].x = hhg.x; }
                            if (s1) { H[j].y = hh.y; F[j].y = INF.y; Hg[j].y = hhg.y; }
                        }
                        if (s0) { c0[0] = c0i[0]; c1[0] = c1i[0]; }
                        if (s1) { c0[1] = c0i[1]; c1[1] = c1i[1]; }
                    }
                }
                // the row's pattern symbols / mismatch scores, the text symbols entering column 30, and the row's mismatch flags:
                // nq(u) bit 30-j = column j of alignment u does NOT match (31 columns from the two planes; an N in the read matches
                // nothing; a column-30 symbol past the text end is the 255 sentinel for this row and a 3 once it is in the cache).
                // (A half that has no rows left -- or never had any -- keeps computing on whatever its streams hold: nothing of it
                // is reported.)
                uint32_t nq[2]; int S[2];
                if (has_quals)
                {
                    #pragma unroll
                    for (int u = 0; u < 2; ++u)
                    {
                        const uint32_t ql = (uint32_t)(qchunk[u] >> qsh[u]) & 0xFFu; qsh[u] += qstep[u];
                        S[u] = s_mm[ql < 63u ? ql : 63u];
                    }
                }
                else S[0] = S[1] = S_noq;
                #pragma unroll
                for (int u = 0; u < 2; ++u)
                {
                    const uint32_t q = ((rchunk[u] >> rsh[u]) & RMASK) ^ cx[u]; rsh[u] += rstep[u];     // (complementing keeps an N an N)
                    c1[u] = __builtin_amdgcn_alignbit( c1[u], tchunk[u],  31 );
                    c0[u] = __builtin_amdgcn_alignbit( c0[u], tchunk1[u], 31 );
                    tchunk[u] <<= 2; tchunk1[u] <<= 2;
                    uint32_t x = (c0[u] ^ (0u - (q & 1u))) | (c1[u] ^ (0u - ((q >> 1) & 1u)));
                    if (RBITS > 2 && q >= 4u) x = 0xFFFFFFFFu;
                    if (i >= (RAGGED ? lim[u] + pad[u] : lim[u])) x |= 1u;      // column 30 past the text end
                    nq[u] = x;
                }
                // both alignments side by side: column j >= 15 at bits 30-j / 46-j of NWa, column j < 15 at bits 14-j / 30-j of NWb
                const uint32_t NWa = __builtin_amdgcn_perm( nq[1], nq[0], 0x05040100u );
                const uint32_t NWb = __builtin_amdgcn_perm( nq[1], nq[0], 0x07060302u );

                // M0 (match = 0): d = H + mismatch * S; else d = (H + V) + mismatch * (S - V); FP: the flag is 2^-7, the penalty S * 128
                const v2 SS = FP ? pk_of<v2>( S[0] * 128, S[1] * 128 ) : pk_of<v2>( S[0], S[1] );
                const v2 SD = pk_of<v2>( S[0] - V, S[1] - V );
                const v2 VV = pk_of<v2>( V, V );
                // column j's pair of mismatch flags: bits 30-j / 46-j of NWa (j >= 15) or 14-j / 30-j of NWb (j < 15), moved to bit 0 (13 with FP)
                // of each half
                auto flags_at = [&](const int j) -> uint32_t {                // ... moved into place,
                    const uint32_t w = (j < 15) ? NWb : NWa;
                    const int bit = (j < 15) ? 14 - j : 30 - j;              // of the low half
                    const int to  = FP ? 13 : 0;
                    return bit >= to ? w >> (bit - to) : w << (to - bit);
                };
                auto flags_in = [&](const uint32_t q) -> v2 { return __builtin_bit_cast( v2, q & (FP ? 0x20002000u : 0x00010001u) ); };   // ... and masked
                auto flags_of = [&](const int j) -> v2 { return flags_in( flags_at( j ) ); };
                auto diag_of = [&](const v2 h, const v2 t) -> v2 {
                    if (FP) return __builtin_bit_cast( v2, __builtin_elementwise_fma( __builtin_bit_cast( v2h, t ), __builtin_bit_cast( v2h, SS ), __builtin_bit_cast( v2h, h ) ) );
                    return M0 ? h + t * SS : (h + VV) + t * SD;
                };

                // One cell is 10 operations: f = max(F[j+1] + GE, Hg[j+1]); d = H[j] + mismatch * S; t = max(f, d); h = max(t, E);
                // hg = h + GO; E' = max(hg, E + GE) -- 9 with FP, where h = max(f, d, E) is one operation.  Only E runs along the row; gfx950
                // needs one idle slot between a packed 16-bit operation and a consumer issued right behind it, so the row is software-pipelined by
                // hand: the E steps of cell j are interleaved with everything of cell j+1 that does not depend on E, in an order in which no
                // operation directly follows its producer (sched_barrier keeps the compiler from undoing it: measured 15 -> 10 issue slots per cell).
                v2 E = ZERO, a = ZERO, tt, ff = INF, dd = ZERO;              // (FP carries f and d of the next cell instead of their maximum)
                v2s key = pk( -1, -1 );
                {
                    // (narrow: what the row before sends into column LO - 1 of this row, before F[LO] is overwritten)
                    if (NARROW && LO > 0) mon = pk_max3( mon, Hg[LO], F[LO] + GE );
                    const v2 x  = F[LO + 1] + GE;
                    const v2 t0 = flags_of( LO );
                    const v2 d  = diag_of( H[LO], t0 );
                    const v2 f  = pk_max( x, Hg[LO + 1] );
                    F[LO] = f;
                    if (FP) { ff = f; dd = d; tt = ZERO; }
                    else
                    {
                        tt = pk_max( f, d );
                        if (TYPE == NVBIO_LOCAL) tt = pk_max( tt, ZERO );
                    }
                }
                #pragma unroll
                for (int j = LO; j <= HI; ++j)
                {
                    constexpr int Z = 0;
                    const int j1 = j + 1, j2 = j + 2;
                    v2 x = INF, d = ZERO, f = INF, t1 = ZERO, tn = ZERO, an = ZERO;
                    uint32_t q1 = 0;
                    if (j2 <= HI) x  = F[j2] + GE;
                    __builtin_amdgcn_sched_barrier( Z );
                    const v2 h = FP ? ((j == LO) ? pk_max( ff, dd ) : pk_max3( ff, dd, E )) : ((j == LO) ? tt : pk_max( tt, E ));
                    if (j1 <= HI) q1 = flags_at( j1 );
                    __builtin_amdgcn_sched_barrier( Z );
                    const v2 hg = h + GO;
                    if (!FP && j1 <= HI) t1 = flags_in( q1 );
                    if (j2 <= HI) f  = pk_max( x, Hg[j2] );
                    __builtin_amdgcn_sched_barrier( Z );
                    const v2 En = (j == LO) ? hg : pk_max( hg, a );
                    if (FP) __builtin_amdgcn_sched_barrier( Z );            // (one cell is an operation shorter: keep E' away from its consumer)
                    if (FP && j1 <= HI) t1 = flags_in( q1 );
                    if (j1 <= HI) d  = diag_of( H[j1], t1 );
                    __builtin_amdgcn_sched_barrier( Z );
                    if (j1 <= HI) an = En + GE;
                    if (NARROW && HI < BAND - 1 && j == HI) mon = pk_max( mon, En );      // (narrow: what column HI sends into column HI + 1)
                    if (TYPE == NVBIO_LOCAL) key = pk_max( key, __builtin_bit_cast( v2s, h ) * K32 + pk( j, j ) );
                    __builtin_amdgcn_sched_barrier( Z );
                    if (j1 <= HI)
                    {
                        if (FP) { ff = (j2 <= HI) ? f : d; dd = d; }
                        else
                        {
                            tn = (j2 <= HI) ? pk_max( f, d ) : d;
                            if (TYPE == NVBIO_LOCAL) tn = pk_max( tn, ZERO );
                        }
                        F[j1] = f;
                    }
                    H[j] = h; Hg[j] = hg;
                    E = En; a = an; tt = tn;
                    __builtin_amdgcn_sched_barrier( Z );
                }

                if (TYPE == NVBIO_LOCAL)
                {
                    // BestSink: row-major reports, the LAST maximum wins
                    const int k0 = key.x, k1 = key.y;
                    if (i < rows_u[0] && (k0 >> 5) >= best[0]) { best[0] = k0 >> 5; best_x[0] = i + (uint32_t)(k0 & 31) + 1u; best_y[0] = i + 1u; }
                    if (i < rows_u[1] && (k1 >> 5) >= best[1]) { best[1] = k1 >> 5; best_x[1] = i + (uint32_t)(k1 & 31) + 1u; best_y[1] = i + 1u; }
                }
            }
            };
            chunk_rows( LO_, HI_ );
        };
        typedef std::integral_constant<int,0> C0; typedef std::integral_constant<int,BAND - 1> C30;
        if (NARROW && ROLE != 0 && rows > NARROW_FULL_ROWS)
        {
            // (two loops, so that the narrow body's loop invariants are set up behind the full-band rows, where registers are free)
            typedef std::integral_constant<int,15 - NARROW_A_HALF> ALO; typedef std::integral_constant<int,15 + NARROW_A_HALF> AHI;
            typedef std::integral_constant<int,15 - NARROW_B_HALF> BLO; typedef std::integral_constant<int,15 + NARROW_B_HALF> BHI;
            // the qualification: every outer H and F of a half must be below its L -- they join what the monitor has seen, which is held
            // against L at the end -- and become the infimum.  (A lane that splits its two alignments over two passes is simply redone:
            // 0 is below no L.)
            auto qualify = [&](auto LO_, auto HI_)
            {
                constexpr int LO = decltype(LO_)::value, HI = decltype(HI_)::value;
                #pragma unroll
                for (int j = 0; j < BAND; ++j)
                    if (j < LO || j > HI)
                    {
                        mon = pk_max3( mon, H[j], F[j] );
                        H[j] = INF; Hg[j] = INF; F[j] = INF;
                    }
                if (split) mon = ZERO;
            };
            for (uint32_t r0 = 0; r0 < NARROW_FULL_ROWS; r0 += 8u) do_chunk( r0, C0(), C30() );
            if (ROLE == 2) { qualify( ALO(), AHI() ); for (uint32_t r0 = NARROW_FULL_ROWS; r0 < rows; r0 += 8u) do_chunk( r0, ALO(), AHI() ); }
            else           { qualify( BLO(), BHI() ); for (uint32_t r0 = NARROW_FULL_ROWS; r0 < rows; r0 += 8u) do_chunk( r0, BLO(), BHI() ); }
        }
        else
            for (uint32_t r0 = 0; r0 < rows; r0 += 8u) do_chunk( r0, C0(), C30() );

        // ---- end-of-alignment reports (:624-645); every active half ended at row `rows` (or has no rows) ----
        if (TYPE != NVBIO_LOCAL)
        {
            #pragma unroll
            for (int u = 0; u < 2; ++u)
            {
                const bool active = (u ? want1 : want0) && (!split || u == pass);
                if (!active) continue;
                if (TYPE == NVBIO_GLOBAL)
                {
                    const int v = u ? (int)H[BAND - 1].y : (int)H[BAND - 1].x;
                    if (best[u] <= v) { best[u] = v; best_x[u] = M[u] + BAND - 1; best_y[u] = M[u]; }
                }
                else
                {
                    const uint32_t mb = M[u] + (uint32_t)(BAND - 1);
                    const uint32_t m  = (mb < N[u] ? mb : N[u]) - (M[u] - 1u);
                    #pragma unroll
                    for (int j = 0; j < BAND; ++j)
                        if (j == 0 || (uint32_t)j < m)
                        {
                            const int v = u ? (int)H[j].y : (int)H[j].x;
                            if (best[u] <= v) { best[u] = v; best_x[u] = M[u] + j; best_y[u] = M[u]; }
                        }
                }
            }
        }
    }
    };
    if (NARROW && role == 1)      run_passes( std::integral_constant<int,1>() );
    else if (NARROW && role == 2) run_passes( std::integral_constant<int,2>() );
    else                          run_passes( std::integral_constant<int,0>() );
    #pragma unroll
    for (int u = 0; u < 2; ++u)
    {
        if (!valid[u]) continue;
        // (narrow: L is the first pass's stash; it is < 0, and a half that ran no narrow row has seen nothing)
        if (NARROW && role != 0 && !((u ? (float)mon.y : (float)mon.x) < (float)scores[out_id[u]]))
        {
            nj.redo[atomicAdd( nj.redo_count, 1u )] = out_id[u];     // (rare; scores[] keeps the stash)
            continue;
        }
        scores[out_id[u]] = best[u]; sinks[out_id[u]] = make_uint2( best_x[u], best_y[u] );
    }
}

// the packed kernel is exact iff no intermediate value can leave the int16 range or meet the -16384 stand-in
// for the reference's infimum: LOCAL additionally packs (score << 5 | column), so scores must fit 10 bits
bool packed_ok(const int type, const SchemeDev& sc, const uint32_t max_read_len)
{
    if (max_read_len == 0) return false;
    const int lim = 4096;
    if (sc.mm_min < 0 || sc.mm_max < 0 || sc.mm_min > lim || sc.mm_max > lim) return false;
    if (sc.pat_go > 0 || sc.pat_ge > 0 || sc.pat_go < -lim || sc.pat_ge < -lim) return false;
    if (sc.match < 0) return false;
    if (type == NVBIO_LOCAL) return (uint64_t)sc.match * max_read_len <= 1000u;
    if (sc.txt_go > 0 || sc.txt_ge > 0 || sc.txt_go < -lim || sc.txt_ge < -lim) return false;
    // |score| <= (rows + band) * (largest single step) must stay far from -16384
    return ((int64_t)max_read_len + 32) * scheme_max_step( sc ) <= 8000;
}

// the binary16 build is exact while every score stays an integer of magnitude <= 2040 (and the scaled penalties finite)
bool pk_binary16_ok(const int type, const BatchDev& b, const SchemeDev& sc)
{
    const bool two = (b.algo & NVBIO_ALN_PK_THREE_WAVES) == 0;
    return two && sc.match == 0 && type == NVBIO_SEMI_GLOBAL && !(b.algo & NVBIO_ALN_NO_F16_DP) && ((int64_t)b.max_read_len + 32) * scheme_max_step( sc ) <= 2040 && sc.mm_max <= 400;
}

// One build of the packed kernel (its template arguments but the read bits), as one number for with_value
struct PkVariant
{
    int type, minw; bool m0, ragged, fp, narrow;
    constexpr int code() const { return type | (minw << 2) | (m0 << 4) | (ragged << 5) | (fp << 6) | (narrow << 7); }
    static constexpr PkVariant of(const int c) { return PkVariant{ c & 3, (c >> 2) & 3, ((c >> 4) & 1) != 0, ((c >> 5) & 1) != 0, ((c >> 6) & 1) != 0, ((c >> 7) & 1) != 0 }; }
};
constexpr int pk_build(const int type, const int minw, const bool m0, const bool ragged = false, const bool fp = false, const bool narrow = false)
{
    return PkVariant{ type, minw, m0, ragged, fp, narrow }.code();
}
// the builds that exist, each for 4- and 2-bit reads: 14 x 2 instantiations
using PkBuilds = Values<
    pk_build( NVBIO_GLOBAL, 2, false ),      pk_build( NVBIO_GLOBAL, 3, false ),
    pk_build( NVBIO_LOCAL, 2, false ),       pk_build( NVBIO_LOCAL, 3, false ),
    pk_build( NVBIO_SEMI_GLOBAL, 2, false ), pk_build( NVBIO_SEMI_GLOBAL, 3, false ),
    pk_build( NVBIO_GLOBAL, 2, true ),       pk_build( NVBIO_GLOBAL, 3, true ),               // match = 0: one operation less per cell
    pk_build( NVBIO_SEMI_GLOBAL, 2, true ),  pk_build( NVBIO_SEMI_GLOBAL, 3, true ),
    pk_build( NVBIO_SEMI_GLOBAL, 2, true, false, true ),                                     // binary16 (the GLOBAL kernel's binary16 build spills: SEMI_GLOBAL only)
    pk_build( NVBIO_SEMI_GLOBAL, 2, true, true ), pk_build( NVBIO_SEMI_GLOBAL, 2, true, true, true ),      // ragged reads, int16 and binary16
    pk_build( NVBIO_SEMI_GLOBAL, 2, true, false, true, true )>;                              // the narrow roles

// the packed kernel's build for this type, scheme and batch: match = 0 (every end-to-end scheme of nvBowtie) drops one operation per cell
// narrow: the launch over the narrow roles' lists (the caller has checked that the binary16 build runs and that the batch is not declared ragged)
static PkVariant pk_variant(const int type, const BatchDev& b, const SchemeDev& sc, const bool narrow)
{
    const int  minw = (b.algo & NVBIO_ALN_PK_THREE_WAVES) ? 3 : 2;
    const bool fp = pk_binary16_ok( type, b, sc ), m0 = sc.match == 0;
    if (narrow) return PkVariant{ NVBIO_SEMI_GLOBAL, 2, true, false, true, true };
    // reads of different lengths (the caller says so): both alignments of a lane in one pass
    if (type == NVBIO_SEMI_GLOBAL && m0 && (b.algo & NVBIO_ALN_RAGGED_READS)) return PkVariant{ NVBIO_SEMI_GLOBAL, 2, true, true, fp, false };
    if (type != NVBIO_LOCAL && m0) return fp ? PkVariant{ NVBIO_SEMI_GLOBAL, 2, true, false, true, false } : PkVariant{ type, minw, true, false, false, false };
    return PkVariant{ type, minw, false, false, false, false };
}

nvbio_status launch_pk_kernel(const int type, const uint32_t rbits, const BatchDev& b, const SchemeDev& sc, const uint32_t pairs, int32_t* scores, uint2* sinks,
                              const uint32_t* job_list, const uint32_t* job_count, hipStream_t s, const NarrowJobs* narrow)
{
    // (narrow: the three lists are disjoint, so their workgroups are at most the whole batch's and one more per list for the ceilings)
    const dim3 grid( (pairs + 127u) / 128u + (narrow ? 2u : 0u) ), block( 128 );
    const NarrowJobs nj = narrow ? *narrow : NarrowJobs{};
    auto miss = [&] { set_error( "packed band-31 scoring: type %d, read_bits %u not instantiated", type, rbits ); return NVBIO_ERR_UNSUPPORTED; };
    return with_value( PkBuilds(), pk_variant( type, b, sc, narrow != nullptr ).code(), [&](auto CODE)
    {
        return with_value( ReadBits31(), (int)rbits, [&](auto RB)
        {
            constexpr PkVariant v = PkVariant::of( decltype(CODE)::value );
            return NVB_LAUNCH( (banded_gotoh_band31_pk_kernel<v.type,RB,v.minw,v.m0,v.ragged,v.fp,v.narrow>), grid, block, s, b, sc, scores, sinks, job_list, job_count, nj );
        }, miss );
    }, miss );
}

// the packed band-31 end-to-end kernel over a job list, for the full-matrix scorer's narrow route (gotoh_full.hip): 4- or 2-bit reads in a
// 2-bit text, SEMI_GLOBAL; `max_jobs` bounds the list's length (which stays on the device)
bool banded31_packed_ok(const SchemeDev& sc, const uint32_t max_read_len)
{
    return plain_gotoh( sc ) && packed_ok( NVBIO_SEMI_GLOBAL, sc, max_read_len );
}
nvbio_status banded31_packed_launch(const BatchDev& b, const SchemeDev& sc, const uint32_t read_bits, const uint32_t max_jobs, int32_t* scores, uint2* sinks,
                                    const uint32_t* job_list, const uint32_t* job_count, hipStream_t s)
{
    return launch_pk_kernel( NVBIO_SEMI_GLOBAL, read_bits == 4 ? 4u : 2u, b, sc, (max_jobs + 1u) / 2u, scores, sinks, job_list, job_count, s );
}

} // namespace nvbio_amd
