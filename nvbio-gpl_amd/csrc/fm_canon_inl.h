// ---------------------------------------------------------------------------------------------
// fm_canon_inl.h -- the two-strand seed pass over a CANONICAL k-mer table (included by fm_index.hip, inside namespace nvbio_amd).
//
// What is computed: for every seed window S of a read, match() of S (the forward strand) AND match() of its reverse complement
// (nvBowtie searches both, mapping_inl.h:288-414; the fmmap-shaped pipeline runs the seed pass once per strand with
// NVBIO_FM_SCAN_FORWARD | NVBIO_FM_COMPLEMENT), each followed by locate() of a search that ends on one row -- the outputs of two
// launches of the per-strand pass (fm_seed_pipe_kernel), from ONE table gather per window instead of one per window and strand.
//
// How.  Let k = ckmer (odd), r = len - k, W = the last k symbols of S and A = its first r symbols (S = A W).  An occurrence of W in the
// text at p is a forward hit at p - r iff text[p-r, p) = A; an occurrence of rc(W) at p is a reverse-strand hit at p iff
// text[p+k, p+k+r) = rc(A) (rc(S) = rc(W) rc(A)).  W and rc(W) share ONE table entry -- the entry of whichever of the two has its
// middle symbol in {A, C} (k is odd: the middle symbols of W and rc(W) are complements, so exactly one qualifies; dropping that
// symbol's high bit gives a dense index of 2^(2k-1) entries: 64 GiB at k = 17 where the per-strand table takes 128) -- and that
// entry lists the occurrences of BOTH orientations, each with the 7 text symbols before and the 7 after it, taken in the
// orientation of the canonical k-mer C:
//   entry (lo, hi):  hi <  MARK, lo >  hi : no occurrence of either orientation
//                    hi <  MARK, lo <= hi : more than 8 occurrences: the search falls back to rank steps (per strand)
//                    hi >= MARK, lo <  MARK : ONE occurrence: lo = text position p of the k-mer,
//                                             hi - MARK = o << 28 | before << 14 | after, where o = 0 if text[p, p+k) = C and 1 if it is
//                                             rc(C); before[t] (bits 2(6-t) of the field) = the symbol t+1 places before C in C's
//                                             orientation: text[p-1-t] (o = 0) or 3 - text[p+k+t] (o = 1); after[t] likewise the symbol
//                                             t+1 places after C: text[p+k+t] (o = 0) or 3 - text[p-1-t] (o = 1); symbols outside the
//                                             text read as 0 and are never trusted (the position checks below exclude them)
//                    hi >= MARK, lo >= MARK : m = hi - MARK in 2..8 occurrences, rows (position, MARK | payload) at cside + 4 (lo - MARK):
//                                             2..4 rows in 32 bytes, 5..8 in 64 (aligned): the occurrences of C in SA order, then those of rc(C)
// A window whose last k symbols are W looks up C = W (qo = 0) or C = rc(W) (qo = 1).  Row (p, o): it is an occurrence of W if o = qo and of
// rc(W) otherwise; qo = 0 compares `before` with A reversed (the seed's remaining symbols in scan order), qo = 1 compares `after` with their
// complement (rc(A) follows C = rc(W)).  A forward hit needs p >= r, a reverse one p + len <= length.
//
// Entries of 16 bytes (NVBIO_FM_TABLE_CANONICAL_WIDE, 128 GiB at k = 17): two slots.  Slot 0 is as above; a k-mer with exactly TWO
// occurrences has the second row in slot 1 (hi >= MARK there; (0, 0) otherwise), and groups begin at three occurrences (3..4 rows in 32
// bytes, 5..8 in 64).  On a 3 Gbp text one seed window in four has a k-mer that occurs once more somewhere, in either orientation:
// 1.25 gathered sectors per window with 8-byte entries, 1.04 with 16-byte ones.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t CTAB_FLANK    = 7u;            // symbols stored on each side of an occurrence: seeds of up to k + 7 symbols
constexpr uint32_t CTAB_ROWS_MAX = 8u;
constexpr uint32_t CTAB_INLINE   = 4u;            // a seed with up to this many hits on a strand can leave them all as keys (inline_max)

__device__ __forceinline__ uint64_t canon_revcomp(const uint64_t key, const uint32_t k)
{
    return reverse_symbols( key, k ) ^ ((1ull << (2u * k)) - 1ull);
}
__device__ __forceinline__ uint64_t canon_index(const uint64_t ckey, const uint32_t k)      // ckey: bit k (middle symbol's high bit) is 0
{
    return ((ckey >> (k + 1u)) << k) | (ckey & ((1ull << k) - 1ull));
}
__device__ __forceinline__ uint64_t canon_key(const uint64_t idx, const uint32_t k)
{
    return ((idx >> k) << (k + 1u)) | (idx & ((1ull << k) - 1ull));
}
__device__ __forceinline__ uint32_t text_symbol(const uint32_t* __restrict__ text, const uint32_t i)
{
    return (text[i >> 4] >> (30u - 2u * (i & 15u))) & 3u;
}

// the SA range of the k-mer `key` (scan order) from the table of (k-1)-mers: one search step, as fm_ktab_level_kernel
__device__ __forceinline__ uint2 canon_range(const DevIndex& f, const uint64_t key)
{
    const uint2 r = f.ktab[key >> 2];
    uint32_t x = r.x, y = r.y, nb = 0;
    if (x <= y) search_step<false>( f, x, y, (uint32_t)(key & 3u), nb );
    return make_uint2( x, y );
}
__device__ __forceinline__ uint32_t range_rows(const uint2 r) { return r.x <= r.y ? r.y - r.x + 1u : 0u; }

// 0: empty / heavy   1: in the entry itself (one occurrence; two with 16-byte entries)   2: up to 4 rows (4 slots)   3: 5..8 (8 slots)
__device__ __forceinline__ uint32_t canon_class(const uint32_t m, const bool wide)
{
    if (m == 1u || (wide && m == 2u)) return 1u;
    return m >= 2u && m <= 4u ? 2u : (m >= 5u && m <= CTAB_ROWS_MAX ? 3u : 0u);
}

// the row of an occurrence: o = 0: text[p, p+k) is the canonical k-mer; o = 1: its reverse complement
__device__ __forceinline__ uint2 canon_row(const uint32_t* __restrict__ text, const uint32_t length, const uint32_t k, const uint32_t p, const uint32_t o)
{
    uint32_t before = 0, after = 0;
    #pragma unroll
    for (uint32_t t = 0; t < CTAB_FLANK; ++t)
    {
        const bool has_l = p >= t + 1u, has_r = (uint64_t)p + k + t < length;
        const uint32_t l = has_l ? text_symbol( text, p - 1u - t ) : 0u;
        const uint32_t g = has_r ? text_symbol( text, p + k + t ) : 0u;
        const uint32_t b = o ? (has_r ? 3u - g : 0u) : l;
        const uint32_t a = o ? (has_l ? 3u - l : 0u) : g;
        before |= b << (2u * (CTAB_FLANK - 1u - t));
        after  |= a << (2u * (CTAB_FLANK - 1u - t));
    }
    return make_uint2( p, DTAB_MARK | (o << 28) | (before << 14) | after );
}

// pass 1: tab[idx] = SA range of the reverse complement of canonical k-mer idx (kept for pass 2); per-tile group counts
__global__ void __launch_bounds__(256)
fm_ctab_count_kernel(const DevIndex f, const uint32_t k, const uint32_t wide, uint2* __restrict__ tab, const uint64_t n, const uint32_t n_tiles,
                     uint32_t* __restrict__ cnt_small, uint32_t* __restrict__ cnt_large)
{
    const uint32_t stride = wide ? 2u : 1u;                      // slots per entry
    __shared__ uint32_t s_a[4], s_b[4];
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    {
        const uint64_t e0 = (uint64_t)tile * DT_TILE + threadIdx.x * 4u;
        uint32_t a = 0, b = 0;
        #pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
            if (e0 + j < n)
            {
                const uint64_t key = canon_key( e0 + j, k );
                const uint2 r1 = canon_range( f, key ), r2 = canon_range( f, canon_revcomp( key, k ) );
                tab[(e0 + j) * stride] = r2;
                const uint32_t c = canon_class( range_rows( r1 ) + range_rows( r2 ), wide != 0u );
                a += (c == 2u); b += (c == 3u);
            }
        a = wave_inclusive_sum( a ); b = wave_inclusive_sum( b );
        if ((threadIdx.x & 63u) == 63u) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
        __syncthreads();
        if (threadIdx.x == 0) { cnt_small[tile] = s_a[0] + s_a[1] + s_a[2] + s_a[3]; cnt_large[tile] = s_b[0] + s_b[1] + s_b[2] + s_b[3]; }
        __syncthreads();
    }
}

// pass 2: the entries and the groups; large groups occupy side slots [0, 8 tot_large), small ones follow
__global__ void __launch_bounds__(256)
fm_ctab_fill_kernel(const DevIndex f, const uint32_t k, const uint32_t wide, uint2* __restrict__ tab, const uint64_t n, const uint32_t n_tiles,
                    const uint32_t* __restrict__ off_small, const uint32_t* __restrict__ off_large, const uint32_t tot_large, uint2* __restrict__ side)
{
    __shared__ uint32_t s_a[4], s_b[4];
    const uint32_t stride = wide ? 2u : 1u;
    auto position = [&](const uint32_t row) -> uint32_t { const uint32_t sv = f.ssa[row]; return sv == 0xFFFFFFFFu ? f.length : sv; };
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    {
        const uint64_t e0 = (uint64_t)tile * DT_TILE + threadIdx.x * 4u;
        uint2 r1[4], r2[4]; uint32_t c[4];
        uint32_t a = 0, b = 0;
        #pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
        {
            c[j] = 0u; r1[j] = r2[j] = make_uint2( 1u, 0u );
            if (e0 + j < n)
            {
                r1[j] = canon_range( f, canon_key( e0 + j, k ) ); r2[j] = tab[(e0 + j) * stride];
                c[j] = canon_class( range_rows( r1[j] ) + range_rows( r2[j] ), wide != 0u );
                a += (c[j] == 2u); b += (c[j] == 3u);
            }
        }
        const uint32_t ia = wave_inclusive_sum( a ), ib = wave_inclusive_sum( b );
        if ((threadIdx.x & 63u) == 63u) { s_a[threadIdx.x >> 6] = ia; s_b[threadIdx.x >> 6] = ib; }
        __syncthreads();
        uint32_t ga = ia - a, gb = ib - b;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) { ga += s_a[w]; gb += s_b[w]; }
        ga += off_small[tile]; gb += off_large[tile];
        __syncthreads();
        #pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
        {
            if (e0 + j >= n) continue;
            const uint32_t n1 = range_rows( r1[j] ), n2 = range_rows( r2[j] ), m = n1 + n2;
            uint2* ent = tab + (e0 + j) * stride;
            if (wide) ent[1] = make_uint2( 0u, 0u );                         // no second row
            auto occurrence = [&](const uint32_t s) -> uint2 {               // row s of the entry: the occurrences of C in SA order, then those of rc(C)
                return s < n1 ? canon_row( f.text, f.length, k, position( r1[j].x + s ), 0u )
                              : canon_row( f.text, f.length, k, position( r2[j].x + (s - n1) ), 1u );
            };
            if (c[j] == 1u)
            {
                ent[0] = occurrence( 0u );
                if (m == 2u) ent[1] = occurrence( 1u );
            }
            else if (c[j] >= 2u)
            {
                const uint32_t slots = c[j] == 2u ? 4u : 8u;
                const uint32_t idx4  = c[j] == 2u ? 2u * tot_large + ga++ : 2u * gb++;
                uint2* g = side + 4ull * idx4;
                for (uint32_t s = 0; s < slots; ++s) g[s] = s < m ? occurrence( s ) : make_uint2( 0u, DTAB_MARK );
                ent[0] = make_uint2( DTAB_MARK | idx4, DTAB_MARK | m );
            }
            else ent[0] = m ? make_uint2( 0u, 1u ) : make_uint2( 1u, 0u );             // heavy : empty
        }
    }
}

// the canonical table of k-mers from the plain table of (k-1)-mers the handle keeps (idx->ktab)
static nvbio_status build_canonical_table(FMIndexImpl* idx, const uint32_t k, const bool wide, hipStream_t stream)
{
    const uint32_t length = idx->view.length;
    if ((uint64_t)length + 2u > DTAB_MARK) { set_error( "canonical table: the text is too long for the position marker" ); return NVBIO_ERR_UNSUPPORTED; }
    const uint64_t entries = 1ull << (2u * k - 1u);
    const uint32_t n_tiles = (uint32_t)((entries + DT_TILE - 1u) / DT_TILE);
    const dim3 grid( n_tiles < 256u * 64u ? n_tiles : 256u * 64u ), block( 256 );
    uint2* tab = nullptr; uint32_t* cnt = nullptr; void* temp = nullptr; uint2* side = nullptr;
    size_t temp_bytes = 0;
    const uint64_t tab_bytes = entries * sizeof(uint2) * (wide ? 2u : 1u);
    if (hipMalloc( (void**)&tab, tab_bytes ) != hipSuccess) { (void)hipGetLastError(); set_error( "canonical table: out of device memory" ); return NVBIO_ERR_NOMEM; }
    if (hipMalloc( (void**)&cnt, 4ull * n_tiles * sizeof(uint32_t) ) != hipSuccess) { (void)hipGetLastError(); (void)hipFree( tab ); set_error( "canonical table: out of device memory" ); return NVBIO_ERR_NOMEM; }
    uint32_t *cs = cnt, *cl = cnt + n_tiles, *os = cnt + 2ull * n_tiles, *ol = cnt + 3ull * n_tiles;
    const DevIndex f = idx->dev();
    nvbio_status st = NVB_LAUNCH( fm_ctab_count_kernel, grid, block, stream, f, k, wide ? 1u : 0u, tab, entries, n_tiles, cs, cl );
    if (st != NVBIO_OK) { (void)hipFree( cnt ); (void)hipFree( tab ); return st; }
    hipError_t e = hipcub::DeviceScan::ExclusiveSum( nullptr, temp_bytes, cs, os, (int)n_tiles, stream );
    if (e == hipSuccess) e = hipMalloc( &temp, temp_bytes ? temp_bytes : 16 );
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum( temp, temp_bytes, cs, os, (int)n_tiles, stream );
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum( temp, temp_bytes, cl, ol, (int)n_tiles, stream );
    uint32_t last[4] = { 0, 0, 0, 0 };
    if (e == hipSuccess) e = hipMemcpyAsync( &last[0], cs + n_tiles - 1u, 4, hipMemcpyDeviceToHost, stream );
    if (e == hipSuccess) e = hipMemcpyAsync( &last[1], os + n_tiles - 1u, 4, hipMemcpyDeviceToHost, stream );
    if (e == hipSuccess) e = hipMemcpyAsync( &last[2], cl + n_tiles - 1u, 4, hipMemcpyDeviceToHost, stream );
    if (e == hipSuccess) e = hipMemcpyAsync( &last[3], ol + n_tiles - 1u, 4, hipMemcpyDeviceToHost, stream );
    if (e == hipSuccess) e = hipStreamSynchronize( stream );
    if (e != hipSuccess) { (void)hipGetLastError(); set_error( "canonical table: counting pass failed: %s", hipGetErrorString( e ) ); st = NVBIO_ERR_HIP; }
    const uint32_t tot_small = last[0] + last[1], tot_large = last[2] + last[3];
    const uint64_t units = 2ull * tot_large + tot_small;                      // groups in units of 4 slots (32 bytes)
    if (st == NVBIO_OK && units >= (1ull << 30)) { set_error( "canonical table: too many groups" ); st = NVBIO_ERR_UNSUPPORTED; }
    if (st == NVBIO_OK && hipMalloc( (void**)&side, (units ? units : 1u) * 32ull ) != hipSuccess) { (void)hipGetLastError(); set_error( "canonical table: out of device memory" ); st = NVBIO_ERR_NOMEM; }
    if (st == NVBIO_OK)
    {
        st = NVB_LAUNCH( fm_ctab_fill_kernel, grid, block, stream, f, k, wide ? 1u : 0u, tab, entries, n_tiles, (const uint32_t*)os, (const uint32_t*)ol, tot_large, side );
        if (st == NVBIO_OK && hipStreamSynchronize( stream ) != hipSuccess) { set_error( "canonical table: fill pass failed" ); st = NVBIO_ERR_HIP; }
    }
    (void)hipFree( cnt );
    if (temp) (void)hipFree( temp );
    if (st != NVBIO_OK) { (void)hipFree( tab ); if (side) (void)hipFree( side ); return st; }
    idx->ctab = tab; idx->cside = side; idx->ckmer = k; idx->cwide = wide ? 1u : 0u;
    idx->owned_bytes += tab_bytes + (units ? units : 1u) * 32ull;
    return NVBIO_OK;
}

// ---------------------------------------------------------------------------------------------
// a window against the rows of its entry.  The window is V, its len symbols with symbol t at bits [2 t, +2) (seed_bits_from_words, fwd =
// false); qo = 1 if the table holds the reverse complement of its last k symbols; want = its first r = len - k symbols as a flank.
// ---------------------------------------------------------------------------------------------
// is row (P, C) a hit?  rev: of the reverse strand; v: where the window (rev: its reverse complement) begins in the text
__device__ __forceinline__ bool canon_row_hit(const uint32_t P, const uint32_t C, const uint32_t qo, const uint32_t want, const uint32_t fshift,
                                              const uint32_t r, const uint32_t len, const uint32_t length, bool& rev, uint32_t& v)
{
    const uint32_t pay = C - DTAB_MARK;
    const uint32_t o = (pay >> 28) & 1u;
    const uint32_t flank = qo ? (pay & 0x3FFFu) : ((pay >> 14) & 0x3FFFu);
    if ((flank >> fshift) != want) return false;
    rev = (o ^ qo) != 0u;
    if (rev ? ((uint64_t)P + len > length) : (P < r)) return false;
    v = rev ? P : P - r;
    return true;
}

__device__ __forceinline__ uint4 canon_entry(const DevIndex& f, const uint64_t V, const uint32_t len, const bool wide, uint32_t& qo)
{
    const uint32_t k = f.ckmer;
    const uint64_t key = V >> (2u * (len - k));
    qo = (uint32_t)(key >> k) & 1u;
    const uint64_t idx = canon_index( qo ? canon_revcomp( key, k ) : key, k );
    if (wide) return ((const uint4*)f.ctab)[idx];
    const uint2 e = f.ctab[idx];
    return make_uint4( e.x, e.y, 0u, 0u );
}

// The hits of a window among the rows of its entry e, the group gathered here: nf on the forward strand (the last one at vf), nr on the
// reverse strand (at vr).  false: the table does not answer (more than 8 occurrences).  The counting form of fm_seed_both_kernel's stage 3,
// for the two places that only ask "exactly one hit, and where": the builder of the locus lines and the anchor of a read.
struct CanonHits { uint32_t nf, nr, vf, vr; };
__device__ __forceinline__ bool canon_lookup(const DevIndex& f, const uint64_t V, const uint32_t len, const uint32_t qo, const uint4 e, CanonHits& h)
{
    const uint32_t r = len - f.ckmer, rmask = (1u << (2u * r)) - 1u, fshift = 2u * (CTAB_FLANK - r);
    h.nf = h.nr = h.vf = h.vr = 0u;
    if (e.y < DTAB_MARK) return e.x > e.y;
    const uint32_t rest = (uint32_t)V & rmask, want = qo ? (~rest & rmask) : rest;
    auto row = [&](const uint32_t P, const uint32_t C) {
        bool rev; uint32_t v;
        if (!canon_row_hit( P, C, qo, want, fshift, r, len, f.length, rev, v )) return;
        h.nr += rev ? 1u : 0u; h.vr = rev ? v : h.vr;                    // (selects between registers: a store through a chosen
        h.nf += rev ? 0u : 1u; h.vf = rev ? h.vf : v;                    // address would put the struct into scratch)
    };
    if (e.x < DTAB_MARK) { row( e.x, e.y ); if (e.w >= DTAB_MARK) row( e.z, e.w ); }
    else
    {
        const uint32_t m = e.y - DTAB_MARK;
        // a group is 32 bytes (up to 4 rows) or 64: its gathers are issued together and waited for once, not one latency per pair of rows
        const uint4* g4 = (const uint4*)(f.cside + 4ull * (e.x - DTAB_MARK));
        uint4 g[CTAB_ROWS_MAX / 2u];
        g[0] = g4[0]; g[1] = g4[1]; g[2] = g[3] = make_uint4( 0u, 0u, 0u, 0u );
        if (m > 4u) { g[2] = g4[2]; g[3] = g4[3]; }
        #pragma unroll
        for (uint32_t t = 0; t < CTAB_ROWS_MAX; t += 2u)
            if (t < m) { row( g[t >> 1].x, g[t >> 1].y ); if (t + 1u < m) row( g[t >> 1].z, g[t >> 1].w ); }
    }
    return true;
}

// The locus lines (bitplanes.h: the layout) for seeds of len symbols: one wave per unit of 64 text positions.  u[x] = 1 iff the table,
// asked as the seed pass asks it, answers the window T = text[x, x + len) with exactly the forward hit x and no reverse hit, AND answers
// rc(T) with exactly the reverse hit x and no forward hit.  The two lookups read different entries -- T's is that of its last k symbols,
// rc(T)'s that of T's first k -- and a lane of the seed pass holds T when its read lies on the forward strand and rc(T) when it lies on the
// reverse strand: either one with more than 8 occurrences sends the lane to the ordinary search (deferred: another key order), so
// neither may.  Rows are exact (k-mer + flank = the whole window), so u[x] = 1 implies occ(T) + occ(rc(T)) = 1, and the two agree
// wherever neither k-mer is heavy.
__global__ void __launch_bounds__(256)
seed_locus_kernel(const DevIndex f, const uint32_t len, const uint32_t wide, const uint64_t n_units, const uint64_t n_lines, uint64_t* __restrict__ lines)
{
    const uint32_t lane = threadIdx.x & 63u, n = f.length;
    for (uint64_t unit = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); unit < n_units; unit += (uint64_t)gridDim.x * 4u)
    {
        const uint64_t x64 = unit * 64u + lane;
        const uint32_t sym = x64 < n ? text_symbol( f.text, (uint32_t)x64 ) : 0u;
        bool uq = false;
        if (x64 + len <= n)
        {
            const uint32_t x = (uint32_t)x64;
            uint64_t V; uint32_t qo; CanonHits h;
            (void)seed_bits_from_words<2>( load_seed_words<2>( f.text, x, len ), x, len, false, false, V );
            uint4 e = canon_entry( f, V, len, wide != 0u, qo );
            uq = canon_lookup( f, V, len, qo, e, h ) && h.nf == 1u && h.nr == 0u && h.vf == x;
            if (uq)
            {
                const uint64_t R = canon_revcomp( V, len );
                e  = canon_entry( f, R, len, wide != 0u, qo );
                uq = canon_lookup( f, R, len, qo, e, h ) && h.nf == 0u && h.nr == 1u && h.vr == x;
            }
        }
        const uint64_t ub = __ballot( uq ), lo = __ballot( (sym & 1u) != 0u ), hi = __ballot( (sym & 2u) != 0u );
        // unit U is slot U - 2 L of the lines L = U / 2, U / 2 - 1 and (U even) U / 2 - 2: slots U & 1, + 2, + 4
        if (lane < 3u && (unit >> 1) >= lane)
        {
            const uint64_t L = (unit >> 1) - lane, slot = unit - 2u * L;
            if (L < n_lines && slot < SEED_LOCUS_UNITS) { uint64_t* p = lines + L * 16u + 3u * slot; p[0] = lo; p[1] = hi; p[2] = ub; }
        }
    }
}

// The tile loop of fm_seed_both_kernel<.., LOCUS = true> (see there: the path, why its keys are the same, the pipeline).  seed_geom, entry_of
// and resolve_tile are the kernel's own; a stage whose tile does not exist carries lanes without a seed, which load and write nothing.
// RAGGED = false (every read has read_len symbols and q.interval between its seeds): a seed's offset in its read and the read's length
// are loop constants, and no stage carries them.
// What a stage knows about its lane travels as bits of ONE register (LS_*): as separate bools each is a 64-bit lane mask in a scalar
// pair, and the fourteen of them, on top of the kernel's arguments, sent the scalar file spilling into vector lanes inside the loop.
enum : uint32_t { LS_SEED = 1u, LS_OK = 2u, LS_ASKED = 4u, LS_USABLE = 8u, LS_STRAND = 16u,   // has a seed | the seed is clean (no N) | asks the locus | its read is placed | on the reverse strand
                  LS_SETTLED = 32u,                                                          // x 1, x 2: settled on the locus, on the forward / reverse strand
                  LS_BEGIN = 256u };                                                         // x (begin & 15): where the seed begins in its first packed word
template <int BITS, bool COUNT, bool WIDE, bool RAGGED, typename Geom, typename Entry, typename Resolve>
__device__ __forceinline__ void fm_seed_locus_loop(const DevIndex& f, const StringSetDev& q, const SeedTiles& tl, const uint32_t read_len, const void* __restrict__ locus,
                                                   unsigned long long* __restrict__ sectors_out, unsigned int* __restrict__ routes, const uint32_t tile0,
                                                   const uint32_t lane, const uint32_t lr, const uint32_t j, const bool lane_ok,
                                                   const Geom& seed_geom, const Entry& entry_of, const Resolve& resolve_tile)
{
    const uint32_t n_waves = gridDim.x * 4u;
    const uint32_t k = f.ckmer, len = q.fixed_len, n = f.length;
    const uint32_t anchor = lane - j;                                        // the lane of this read's first seed
    const bool     first = j == 0u;
    const uint32_t u_pfw = j * q.interval;                                   // (uniform reads) the seed's offset in its read
    const uint4 none = make_uint4( 1u, 0u, 0u, 0u );                         // the entry of a k-mer without occurrences
    auto qo_of = [&](const uint64_t V) -> uint32_t { return (uint32_t)(V >> (2u * (len - k) + k)) & 1u; };
    auto pfw_of  = [&](const uint32_t v) -> uint32_t { return RAGGED ? v : u_pfw; };
    auto rlen_of = [&](const uint32_t v) -> uint32_t { return RAGGED ? v : read_len; };
    auto add = [&](unsigned int* word, const bool on) {                      // (COUNT) one atomic per wave
        const uint32_t c = (uint32_t)__popcll( __ballot( on ) );
        if (lane == 0 && c) atomicAdd( word, c );
    };
    // per stage: seed bits V, entry e (none: not gathered), the LS_* bits, (ragged reads) the seed's offset in the read, the read's length
    SeedWords W = { 0, 0, 0, 0, 0 }; uint32_t w_pfw = 0, w_rlen = 0, w_fl = 0;                                // words of tile t+3, loaded
    uint64_t aV = 0; uint4 ae = none; uint32_t a_fl = 0, a_pfw = 0, a_rlen = 0;                               // tile t+2: the anchors' entries loaded
    uint64_t lV = 0; uint32_t l_fl = 0, l_pfw = 0, l_rlen = 0;                                                // tile t+1: the locus words loaded
    uint32_t l_x = 0; LocusWords LW = { none.x, none.y, none.z, none.w, 0 };                                  // (in the lanes j = 0, which never ask: the anchor's entry)
    uint64_t cV = 0; uint4 ce = none; uint32_t c_fl = 0, c_pfw = 0, c_rlen = 0;                               // tile t: the remaining entries loaded
    for (uint32_t step = 0; ; ++step)
    {
        const uint64_t t4 = (uint64_t)tile0 + (uint64_t)step * n_waves;                  // the tile whose words this iteration loads
        if (step >= 4u && t4 - 4ull * n_waves >= tl.n_tiles) break;
        // ---- tile t+1: the lane's window against the locus.  The seed as bit planes; its reverse complement is the planes mirrored and inverted ----
        uint32_t settled = 0;
        if (l_fl & LS_ASKED)
        {
            const uint32_t strand = (l_fl / LS_STRAND) & 1u;
            const uint32_t vl = (uint32_t)lV, vh = (uint32_t)(lV >> 32);
            uint32_t plo = squeeze2( vl ) | (squeeze2( vh ) << 16), phi = squeeze2( vl >> 1 ) | (squeeze2( vh >> 1 ) << 16);
            if (strand) { plo = ~(__brev( plo ) >> (32u - len)); phi = ~(__brev( phi ) >> (32u - len)); }
            if (locus_answers( LW, l_x, len, plo, phi )) settled = 1u + strand;
        }
        if (COUNT && routes)
        {
            add( routes + 1, settled != 0u );
            add( routes + 2, (l_fl & LS_SEED) && !first && (l_fl & LS_USABLE) && !settled );
            add( routes + 3, (l_fl & LS_SEED) && !first && !(l_fl & LS_USABLE) );
        }
        // ---- tile t+2: the anchor placed (its group, if its entry points to one, is gathered here), told to the lanes of its read ----
        uint32_t a_hit = 0xFFFFFFFFu, a_strand = 0;
        if (first && (a_fl & LS_OK))
        {
            CanonHits h;
            if (canon_lookup( f, aV, len, qo_of( aV ), ae, h ) && h.nf + h.nr == 1u) { a_strand = h.nr; a_hit = h.nr ? h.vr : h.vf; }
        }
        const uint32_t r_hit = (uint32_t)__shfl( (int)a_hit, (int)anchor ), r_strand = (uint32_t)__shfl( (int)a_strand, (int)anchor );
        const bool usable = r_hit != 0xFFFFFFFFu;
        bool ask = false; uint32_t x = 0, base = 0;                                      // the window's place on the anchor's diagonal; where the read begins
        if (usable && !first && (a_fl & LS_OK) && rlen_of( a_rlen ) <= SEED_LOCUS_MAX_READ)
        {
            const uint32_t p = pfw_of( a_pfw );
            if (r_strand == 0u) { base = r_hit; x = r_hit + p; ask = (uint64_t)r_hit + p + len <= n; }
            else
            {
                const uint32_t span = rlen_of( a_rlen ) - len;                           // (a lane with a seed: p + len <= its read's length)
                base = r_hit >= span ? r_hit - span : 0u; x = r_hit - p; ask = r_hit >= p;
            }
        }
        if (COUNT)
        {
            if (routes) add( routes, first && usable );
            // the read's locus line, once, in its anchor's lane
            const uint64_t asked = __ballot( ask );
            const uint64_t mine = (q.spr >= 64u ? ~0ull : ((1ull << q.spr) - 1ull)) << anchor;
            const uint32_t c = (uint32_t)__popcll( __ballot( first && (asked & mine) != 0ull ) );
            if (lane == 0 && c) atomicAdd( sectors_out, (unsigned long long)c );
        }
        // ---- tile t+3: the seed bits ----
        uint64_t nV = 0; uint32_t n_fl = w_fl;
        if (w_fl & LS_SEED) n_fl |= seed_bits_from_words<BITS>( W, (w_fl / LS_BEGIN) & 15u, len, false, false, nV ) ? LS_OK : 0u;
        const uint32_t n_pfw = w_pfw, n_rlen = w_rlen;
        // ---- the loads of every stage: groups of t | remaining entries of t+1 | locus words of t+2 | anchor entries of t+3 | words of t+4 ----
        const bool c_ok = (c_fl & LS_OK) != 0u;
        const bool is_one   = c_ok && ce.y >= DTAB_MARK && ce.x < DTAB_MARK;
        const bool is_group = c_ok && ce.y >= DTAB_MARK && ce.x >= DTAB_MARK;
        const bool is_heavy = c_ok && ce.y < DTAB_MARK && ce.x <= ce.y;
        uint4 q0 = make_uint4( 0, 0, 0, 0 ), q1 = q0, q2 = q0, q3 = q0;
        if (is_group)
        {
            const uint4* g4 = (const uint4*)(f.cside + 4ull * (ce.x - DTAB_MARK));
            q0 = g4[0]; q1 = g4[1];
            if (ce.y - DTAB_MARK > 4u) { q2 = g4[2]; q3 = g4[3]; }
        }
        // the anchors of t+3 sit in the lanes j = 0, the remaining windows of t+1 in the others: ONE index computation and ONE gather serve both
        uint4 got = none;
        if (first ? (n_fl & LS_OK) != 0u : ((l_fl & LS_OK) && !settled)) { uint32_t qo; got = entry_of( first ? nV : lV, qo ); }
        const uint4 fe = first ? make_uint4( LW.lo0, LW.lo1, LW.hi0, LW.hi1 ) : got;     // (an anchor's entry is read in the lanes j = 0 only)
        // the anchors' entries travel on in the registers the other lanes load their locus words into: a lane j = 0 never asks
        LocusWords nLW = { ae.x, ae.y, ae.z, ae.w, 0 };
        if (ask) load_locus_words( locus, base, x, nLW );
        {
            const uint64_t rid4 = t4 * tl.rpt + lr;
            uint32_t w_begin = 0;
            bool ws = t4 < tl.n_tiles && lane_ok && rid4 < tl.reads;
            if (RAGGED) { if (ws) ws = seed_geom( (uint32_t)rid4, w_begin, w_pfw, w_rlen ); }
            else if (ws) w_begin = (q.offsets ? q.offsets[rid4] : (uint32_t)rid4 * q.stride) + u_pfw;
            if (ws) W = load_seed_words<BITS>( q.symbols, w_begin, len );
            w_fl = ws ? LS_SEED | ((w_begin & 15u) * LS_BEGIN) : 0u;
        }
        // ---- tile t resolved ----
        if (step >= 4u)
        {
            const uint32_t tile = (uint32_t)(t4 - 4ull * n_waves), rid = tile * tl.rpt + lr;
            resolve_tile( tile, rid, (c_fl & LS_SEED) != 0u, cV, ce, c_ok, qo_of( cV ), pfw_of( c_pfw ), rlen_of( c_rlen ), is_one, is_group, is_heavy,
                          q0, q1, q2, q3, (c_fl / LS_SETTLED) & 3u, (uint32_t)cV );
        }
        // (a settled lane has no entry to hold its seed against: where it was settled travels in the seed's place.  resolve_tile then gets
        // that position as V, and what it derives from V -- qo, the flank -- is garbage in such a lane.  That is harmless ONLY because a
        // settled lane gathered nothing: its ce is `none`, so is_one / is_group / is_heavy are false and no row is held against V.  The
        // same holds for what the lanes j > 0 carry in ae, and the lanes j = 0 in LW: stale or foreign words that nothing reads, since
        // an anchor's entry is taken from LW in the lanes j = 0 alone and only a lane that asked reads LW as locus words.)
        cV = settled ? (uint64_t)l_x : lV; ce = fe; c_fl = l_fl | (settled * LS_SETTLED); c_pfw = l_pfw; c_rlen = l_rlen;
        lV = aV; l_pfw = a_pfw; l_rlen = a_rlen; l_x = x; LW = nLW;
        l_fl = (a_fl & (LS_SEED | LS_OK)) | (ask ? LS_ASKED : 0u) | (usable ? LS_USABLE : 0u) | (r_strand ? LS_STRAND : 0u);
        aV = nV; ae = got; a_fl = n_fl; a_pfw = n_pfw; a_rlen = n_rlen;
    }
}

// ---------------------------------------------------------------------------------------------
// the seed pass of both strands: one wave per tile of whole reads, software-pipelined over the tiles a wave owns as
// fm_seed_pipe_kernel (words of tile t+2 | table entry of tile t+1 | resolution of tile t).  A tile has 128 key slots: the keys of the
// forward strand (at most 64), those of the reverse strand right behind them; tile_counts[tile] = both.  Seeds whose k-mer has more than
// 8 occurrences, or with several hits on a strand (a repeat longer than the seed), need the ordinary search of that strand
// (plain table + rank steps + finish on the text): what ends on several rows goes to that strand's residual
// list: ranges / ids [0, cap) forward, [cap, 2 cap) reverse; counts[1], counts[2].
// DEFER = false: that search runs inside this kernel, in the lane that needs it (every wave that holds one such lane pays its ten
//   dependent gathers: fine on a unique-ish genome where one window in 10^5 needs it, 2.6x the kernel's time when 5 % do).
// DEFER = true (NVBIO_FM_DEFER_HEAVY): the lane only records (seed id | strand << 31) in its tile's 128 deferred slots
//   (tile_defer / defer_counts, compacted like the keys); fm_seed_heavy_kernel then runs those searches as a dense launch of their own.
// Ragged reads (q.intervals): read r has its own length (offsets[r+1] - offsets[r]) and seed interval; lane (read, j) holds a seed iff
//   j x interval + len fits the read; q.spr is the largest seed count of a read (the stride of seed ids).
// ---------------------------------------------------------------------------------------------
// WIDE: 16-byte entries (NVBIO_FM_TABLE_CANONICAL_WIDE): a k-mer with TWO occurrences has both rows in its entry, groups start at three
//
// LOCUS (the handle's locus lines, bitplanes.h, built for this seed length): a read's first seed -- its anchor, lane j = 0 -- is looked up
// as ever.  If it has exactly one hit over both strands, that hit places the whole read, and lane j's window would lie at
// x_j = v + p_j (forward strand) or v - p_j (reverse strand; p_j: the seed's offset in the read).  The lane then reads text[x_j, x_j + len)
// and u[x_j] from the read's ONE locus line instead of gathering a table line of its own, and is settled if the text equals its seed S_j
// (reverse strand: rc(S_j)) and u[x_j] = 1.  Why the keys are the same: let T = text[x_j, x_j + len) with u[x_j] = 1.  By the builder's
// test (seed_locus_kernel) the table answers T with the forward hit x_j alone and rc(T) with the reverse hit x_j alone, neither through a
// heavy entry.  A forward lane holds S_j = T, a reverse lane S_j = rc(T): the table gather it skips would have left exactly hits[strand] = 1,
// pos[strand][0] = x_j and nothing on the other strand, which is what the lane sets.  Every other lane -- text differs, u = 0, x_j outside
// [0, n - len], no usable anchor, a read longer than SEED_LOCUS_MAX_READ -- gathers its entry and resolves it as without LOCUS, and the
// emission sees the same hits and positions either way.
// Pipeline with LOCUS: words of tile t+4 | anchor entries of t+3 | locus words of t+2 | the remaining entries of t+1 | groups and resolution
// of t.  Each iteration first computes on what the last one loaded (locus test of t+1, anchor of t+2, seed bits of t+3), then issues the
// loads of all five stages, then resolves tile t.  The anchors of t+3 and the remaining windows of t+1 sit in different lanes (j = 0, j > 0)
// and share one index computation and one gather.  An anchor whose entry points to a group gathers it while it computes -- its two or
// four loads issued together: the one dependent gather outside the schedule, in the iterations where one of the wave's anchors has a
// k-mer with 3..8 occurrences.  The loop is bound by the vector instructions it issues, not by its loads: what it carries
// from stage to stage and what it computes per lane is kept small for that reason.
// Resolution and emission (resolve_tile), two ways.  The COMMON tile -- no lane heavy, every lane with at most one hit over both strands:
// 98.4 % of the headline batch's tiles -- has its rows evaluated by counts (hits, strand and position of the last one; group rows only in
// a wave that holds a group) and its keys of both strands emitted in ONE pass: forward keys to the slots [0, n0), reverse keys behind them,
// a key dropped iff the nearest lower lane with a key on its strand lies in the same read on the same diagonal (which is key equality: see
// there).  Every other tile runs the general code: hits slot by slot, one emission per strand through emit_seed_results, residual and
// deferred entries, the in-line searches.  Same keys in the same order either way; NVBIO_FM_NO_FAST_RESOLVE (resolve_opts) sends every tile
// through the general code, and only the forms named at FAST_FORM hold the common path at all.  paths (COUNT, NVBIO_FM_COUNT_RESOLVE): tiles resolved as common | by the general code.
// routes (COUNT, NVBIO_FM_COUNT_LOCUS): reads with a usable anchor | windows settled on the locus | windows of such reads that gathered
// after all | windows of reads without a usable anchor -- the last three over the windows behind the anchor (j > 0).
// RAGGED (with LOCUS only; the other forms look at q.intervals): the batch has ragged reads.  A form of its own, chosen by the launcher, so
// that uniform reads pay neither the registers nor the instructions of a geometry that is the same for every read.
constexpr uint32_t SEED_RESOLVE_GENERAL = 16u;   // in resolve_opts: every tile takes the general path (NVBIO_FM_NO_FAST_RESOLVE)
template <int BITS, bool COUNT, bool WIDE, bool DEFER, bool LOCUS, bool RAGGED = false>
__global__ void __launch_bounds__(256)
fm_seed_both_kernel(const DevIndex f, const StringSetDev q, const SeedTiles tl, const uint32_t read_len, const uint32_t resolve_opts,
                    uint64_t* __restrict__ tile_keys, uint32_t* __restrict__ tile_counts, uint2* __restrict__ res_ranges,
                    uint32_t* __restrict__ res_ids, const uint32_t res_cap, unsigned int* __restrict__ counts, unsigned long long* __restrict__ sectors_out,
                    uint32_t* __restrict__ tile_defer, uint32_t* __restrict__ defer_counts, const void* __restrict__ locus, unsigned int* __restrict__ routes,
                    unsigned int* __restrict__ paths)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t inline_max = resolve_opts & 15u;                          // resolve_opts: inline_max | SEED_RESOLVE_GENERAL
    // Which forms hold both ways of resolving a tile.  The second way costs 6 to 9 VGPRs, and that costs some forms a wave per SIMD: the
    // locus loop without DEFER (the C++ host's: 95 -> 103 VGPRs, 5 -> 4 waves, measured no faster), the forms over 8-byte entries and the
    // forms for 2-bit reads (6 -> 5, 7 -> 6; not measured).  Only the forms that keep their waves and were measured have it: 4-bit reads,
    // 16-byte entries, DEFER -- the locus loop (uniform and ragged) and the old loop of the step.  Every other form is compiled with the
    // general code alone, as before.  An accounting form (COUNT, compiled without DEFER) accounts for the launch of the same flags: the
    // launcher sets SEED_RESOLVE_GENERAL for it where that launch asked for no DEFER.
    constexpr bool FAST_FORM = BITS == 4 && WIDE && (COUNT || DEFER);
    const bool fast_ok = FAST_FORM && !(resolve_opts & SEED_RESOLVE_GENERAL) && inline_max >= 1u && f.length >= q.fixed_len;
    const uint32_t n_waves = gridDim.x * 4u;
    const uint32_t k = f.ckmer, len = q.fixed_len, r = len - k;
    const uint32_t lr = lane / q.spr, j = lane - lr * q.spr;
    const bool lane_ok = lr < tl.rpt;
    const bool ragged = LOCUS ? RAGGED : (q.intervals != nullptr);
    const uint32_t rmask = (1u << (2u * r)) - 1u;                            // r <= 7
    const uint32_t fshift = 2u * (CTAB_FLANK - r);
    DevIndex fplain = f; fplain.dtab = nullptr; fplain.dkmer = 0;            // the fallback searches use the plain table only

    // the seed of this lane in read rid: where it begins in the symbol stream, its offset in the read, the read's length; false: no such seed
    auto seed_geom = [&](const uint32_t rid, uint32_t& begin, uint32_t& p_fw, uint32_t& rlen) -> bool {
        const uint32_t base = q.offsets ? q.offsets[rid] : rid * q.stride;
        p_fw  = j * (ragged ? q.intervals[rid] : q.interval);
        rlen  = ragged ? q.offsets[rid + 1] - base : read_len;
        begin = base + p_fw;
        return !ragged || p_fw + len <= rlen;
    };
    auto entry_of = [&](const uint64_t V, uint32_t& qo) -> uint4 {
        const uint64_t key = V >> (2u * r);
        qo = (uint32_t)(key >> k) & 1u;
        const uint64_t idx = canon_index( qo ? canon_revcomp( key, k ) : key, k );
        if (WIDE)
        {
            typedef unsigned int u4v __attribute__((ext_vector_type(4)));
            const u4v v = __builtin_nontemporal_load( (const u4v*)f.ctab + idx );
            return make_uint4( v.x, v.y, v.z, v.w );
        }
        const uint2 e = load_table_entry( f.ctab, idx, true );
        return make_uint4( e.x, e.y, 0u, 0u );
    };

    // ---- stage 3b: a tile resolved -- the rows of every lane's entry e (q0 .. q3: its group) into hits, the hits into keys, residual and
    // deferred entries.  settled (LOCUS): 1 + strand of the one hit, at settled_x, of a lane answered from the locus (its e is empty)
    auto resolve_tile = [&](const uint32_t tile, const uint32_t rid, const bool valid, const uint64_t V, const uint4 e, const bool e_valid, const uint32_t qo,
                            const uint32_t c_pfw, const uint32_t c_rlen, const bool is_one, const bool is_group, const bool is_heavy,
                            const uint4 q0, const uint4 q1, const uint4 q2, const uint4 q3, const uint32_t settled, const uint32_t settled_x)
    {
        const uint32_t m = e.y - DTAB_MARK;
        const uint32_t rest = (uint32_t)V & rmask;                           // the seed's first r symbols, reversed (scan order)
        const uint32_t want = qo ? (~rest & rmask) : rest;
        const uint32_t i = rid * q.spr + j;
        uint32_t sectors = (e_valid && !(LOCUS && settled)) ? (is_group ? 2u : 1u) : 0u;
        // ---- the common tile.  The rows of every lane BY COUNTS, as canon_lookup keeps them but leaner still: the number of hits over both
        // strands, and the strand and row position of the last one -- selects between registers, no slots, no branch (canon_row_hit's
        // tests restated without its early returns: the field of the flank that this lane compares, and the orientation bit, read
        // straight from the row's second word, whose mark sits above both).  The group rows run only in a wave that holds a group, rows
        // 4..7 only where one of its groups has them.  Then ONE wave-uniform decision, behind the group rows: the tile is common iff no
        // lane with a clean seed is heavy or has more than one hit over both strands (and one hit may stay in line: inline_max >= 1).
        // Such a tile has no residual entry, no deferred search, no in-line search and at most 64 keys, and every lane holds at most one
        // (strand, position): both strands are emitted in one pass.  Every other tile runs the general code below, which reads none of
        // these registers.
        bool common = false;
        if (fast_ok)
        {
            const uint32_t fsel = (qo ? 0u : 14u) + fshift;                      // where the compared flank begins in a row's second word
            const uint32_t plim = f.length - len + 1u;                           // a reverse-strand hit at P needs P + len <= length (fast_ok: length >= len)
            uint32_t cnt = 0, hit_rev = 0, hit_p = 0;
            auto crow = [&](const bool on, const uint32_t P, const uint32_t C) {
                const uint32_t rev = ((C >> 28) ^ qo) & 1u;
                const bool fits = rev ? P < plim : P >= r;
                const bool hit = on & (__builtin_amdgcn_ubfe( C, fsel, 2u * r ) == want) & fits;
                cnt += hit ? 1u : 0u; hit_rev = hit ? rev : hit_rev; hit_p = hit ? P : hit_p;
            };
            crow( is_one, e.x, e.y );
            if (WIDE) crow( is_one & (e.w >= DTAB_MARK), e.z, e.w );
            if (__ballot( is_group ))
            {
                const uint32_t gm = is_group ? m : 0u;
                crow( 0u < gm, q0.x, q0.y ); crow( 1u < gm, q0.z, q0.w ); crow( 2u < gm, q1.x, q1.y ); crow( 3u < gm, q1.z, q1.w );
                if (__ballot( gm > 4u ))
                {
                    crow( 4u < gm, q2.x, q2.y ); crow( 5u < gm, q2.z, q2.w ); crow( 6u < gm, q3.x, q3.y ); crow( 7u < gm, q3.z, q3.w );
                }
            }
            uint32_t v = hit_rev ? hit_p : hit_p - r;                            // where the window (its reverse complement) begins in the text
            if (LOCUS && settled) { cnt = 1u; hit_rev = settled - 1u; v = settled_x; }
            const bool live = valid && e_valid;
            common = __ballot( live && (is_heavy || cnt > 1u) ) == 0ull;
            if (common)
            {
                // a lane's one key: (uint64) v + 1024 - p, as emit_seed_results forms it
                const bool     has = live && cnt == 1u;
                const uint32_t s = hit_rev;
                const uint32_t p = s ? c_rlen - c_pfw - len : c_pfw;
                const uint64_t diag = (uint64_t)v + 1024u - p;
                const uint64_t key = ((uint64_t)rid << 34) | ((uint64_t)s << 33) | diag;
                // A key is dropped iff it equals that of the nearest lower lane with a key on the same strand.  Two such keys have the same
                // strand bit, so they are equal iff their reads and their diagonals are.  The read: a tile's reads sit in runs of q.spr
                // lanes, so the predecessor lies in this lane's read iff its lane is not below this read's first (lane - j); the read id
                // occupies bits 34 and up, which the diagonal never reaches: v + 1024 < 2^32 (a text has at most 2^32 - 8193 symbols) and
                // p <= 1024 (NVBIO_MAX_SEED_OFFSET), so 0 <= diag < 2^32.  The diagonal: for the same reason its low word IS the diagonal,
                // and one ds_bpermute of that word replaces the two of the whole key.
                const uint64_t below = (1ull << lane) - 1ull;
                const uint64_t m0 = __ballot( has && s == 0u ), m1 = __ballot( has && s != 0u );
                const uint64_t prev_mask = (s ? m1 : m0) & below;
                const int      prev_lane = prev_mask ? 63 - __clzll( (long long)prev_mask ) : 0;
                const uint32_t prev_diag = (uint32_t)__shfl( (int)(uint32_t)diag, prev_lane );
                const bool     dup = prev_mask != 0ull && (uint32_t)prev_lane >= lane - j && prev_diag == (uint32_t)diag;
                const bool     keep = has && !dup;
                // forward keys to the slots [0, n0) in lane order, reverse keys to [n0, n0 + n1)
                const uint64_t k0 = __ballot( keep && s == 0u ), k1 = __ballot( keep && s != 0u );
                const uint32_t n0 = (uint32_t)__popcll( k0 ), n1 = (uint32_t)__popcll( k1 );
                if (keep) tile_keys[(uint64_t)tile * 128u + (s ? n0 + (uint32_t)__popcll( k1 & below ) : (uint32_t)__popcll( k0 & below ))] = key;
                if (lane == 0) { tile_counts[tile] = n0 + n1; if (DEFER) defer_counts[tile] = 0u; }
            }
        }
        if (COUNT && paths && lane == 0) atomicAdd( paths + (common ? 0 : 1), 1u );
        if (!common)
        {
        // ---- every other tile, in general: hits and positions slot by slot, strand by strand
        // per strand: the hits found among the entry's rows (the first CTAB_INLINE positions are kept)
        uint32_t hits[2] = { 0, 0 }, pos[2][CTAB_INLINE] = { { 0, 0, 0, 0 }, { 0, 0, 0, 0 } };
        auto row = [&](const uint32_t P, const uint32_t C) {
            bool rev; uint32_t v;
            if (!canon_row_hit( P, C, qo, want, fshift, r, len, f.length, rev, v )) return;
            #pragma unroll
            for (int s = 0; s < 2; ++s)
                if ((s == 1) == rev)
                {
                    #pragma unroll
                    for (uint32_t t = 0; t < CTAB_INLINE; ++t) pos[s][t] = (hits[s] == t) ? v : pos[s][t];
                    ++hits[s];
                }
        };
        if (is_one) { row( e.x, e.y ); if (WIDE && e.w >= DTAB_MARK) row( e.z, e.w ); }
        else if (is_group)
        {
#define NVB_CROW(jj, P, C) if ((jj) < m) row( (P), (C) );
            NVB_CROW( 0u, q0.x, q0.y ) NVB_CROW( 1u, q0.z, q0.w ) NVB_CROW( 2u, q1.x, q1.y ) NVB_CROW( 3u, q1.z, q1.w )
            NVB_CROW( 4u, q2.x, q2.y ) NVB_CROW( 5u, q2.z, q2.w ) NVB_CROW( 6u, q3.x, q3.y ) NVB_CROW( 7u, q3.z, q3.w )
#undef NVB_CROW
        }
        if (LOCUS && settled)
        {
            hits[0] = settled == 1u; hits[1] = settled == 2u;
            pos[0][0] = pos[1][0] = settled_x;
        }
        uint32_t tile_fill = 0;                                              // keys of this tile written so far: the reverse strand's follow the forward strand's
        uint32_t defer_fill = 0;                                             // deferred searches of this tile recorded so far (DEFER)
        #pragma unroll
        for (int s = 0; s < 2; ++s)
        {
            // what this strand leaves: cnt keys (positions pos[s][0 .. cnt)), or the range (rx, ry) of several rows for the residual list
            uint32_t cnt = (valid && e_valid && !is_heavy && hits[s] <= inline_max) ? hits[s] : 0u;
            uint32_t rx = 1u, ry = 0u;
            bool searched = false, deferred = false;
            const uint32_t sflags = s ? (NVBIO_FM_SCAN_FORWARD | NVBIO_FM_COMPLEMENT) : 0u;
            auto plain_search = [&]() -> bool {                              // the ordinary search of this strand: range (rx, ry) or a position
                uint32_t nblk, sec = 0; bool single = false;
                match_one<BITS,false,true,true>( fplain, q, sflags, f.ktab != nullptr, false, i, rx, ry, nblk, single, &sec );
                sectors += sec; searched = true;
                return single;
            };
            if (valid && e_valid && (is_heavy || hits[s] > inline_max))
            {
                cnt = 0u;
                if (DEFER) deferred = true;
                else if (plain_search()) { pos[s][0] = rx; cnt = 1u; }
                else if (rx <= ry && ry - rx < inline_max)                   // 1 .. inline_max rows: their positions from the suffix array
                {
                    cnt = ry - rx + 1u;
                    #pragma unroll
                    for (uint32_t t = 0; t < CTAB_INLINE; ++t)
                        if (t < cnt) { const uint32_t sv = f.ssa[rx + t]; pos[s][t] = (sv == 0xFFFFFFFFu) ? f.length : sv; }
                    sectors += cnt;
                }
            }
            // a tile's keys of one strand must fit its 64 slots: if the seeds with several keys would overflow them, those seeds go to the
            // residual list instead (a wave-uniform decision; the range of a seed resolved from its entry's rows is searched for then)
            // (counted only in a wave that has such a seed: the common tile, one key per seed at most, skips the five ballots)
            if (__ballot( cnt >= 2u ))
            {
                uint32_t total = (uint32_t)__popcll( __ballot( cnt == 1u ) );
                #pragma unroll
                for (uint32_t t = 0; t < CTAB_INLINE; ++t) total += (uint32_t)__popcll( __ballot( cnt >= 2u && t < cnt ) );
                if (total > 64u && cnt >= 2u)
                {
                    if (DEFER) { deferred = true; rx = 1u; ry = 0u; }
                    else if (!searched) (void)plain_search();
                    cnt = 0u;
                }
            }
            uint64_t* slots = tile_keys + (uint64_t)tile * 128u + tile_fill;
            uint32_t n_out = 0; uint64_t last = ~0ull;
            const uint32_t x1 = cnt == 1u ? pos[s][0] : (cnt == 0u ? rx : 1u), y1 = cnt == 1u ? pos[s][0] : (cnt == 0u ? ry : 0u);
            emit_seed_results( c_pfw, len, c_rlen, (uint32_t)s, lane, valid, cnt == 1u, x1, y1, rid, i, slots, n_out, last,
                               res_ranges + (s ? res_cap : 0u), res_ids + (s ? res_cap : 0u), counts + s );
            // seeds with 2 .. inline_max hits on this strand: their keys behind the tile's one-hit keys, no duplicate removal
            if (__ballot( cnt >= 2u ))
            {
                uint32_t pq = c_pfw;
                if (s) pq = c_rlen - pq - len;
                #pragma unroll
                for (uint32_t t = 0; t < CTAB_INLINE; ++t)
                {
                    const bool on = cnt >= 2u && t < cnt;
                    const uint64_t mk = __ballot( on );
                    if (on) slots[n_out + (uint32_t)__popcll( mk & ((1ull << lane) - 1ull) )] =
                                ((uint64_t)rid << 34) | ((uint64_t)s << 33) | ((uint64_t)pos[s][t] + 1024u - pq);
                    n_out += (uint32_t)__popcll( mk );
                }
            }
            tile_fill += n_out;
            if (DEFER)
            {
                const uint64_t md = __ballot( deferred );
                if (md)
                {
                    if (deferred) tile_defer[(uint64_t)tile * 128u + defer_fill + (uint32_t)__popcll( md & ((1ull << lane) - 1ull) )] = i | ((uint32_t)s << 31);
                    defer_fill += (uint32_t)__popcll( md );
                }
            }
        }
        if (lane == 0) { tile_counts[tile] = tile_fill; if (DEFER) defer_counts[tile] = defer_fill; }
        }
        if (COUNT)
        {
            uint32_t tot = valid ? sectors : 0u;
            #pragma unroll
            for (int d = 32; d > 0; d >>= 1) tot += (uint32_t)__shfl_xor( (int)tot, d );
            if (lane == 0 && tot) atomicAdd( sectors_out, (unsigned long long)tot );
        }
    };

    uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= tl.n_tiles) return;
    if constexpr (LOCUS)
    {
        // (a wave's first tile is the same in every lane: told to the compiler, the tile and step arithmetic of the loop is scalar)
        tile = (uint32_t)__builtin_amdgcn_readfirstlane( (int)tile );
        fm_seed_locus_loop<BITS,COUNT,WIDE,RAGGED>( f, q, tl, read_len, locus, sectors_out, routes, tile, lane, lr, j, lane_ok, seed_geom, entry_of, resolve_tile );
        return;
    }
    // stage 1 -> 2 (the tile after the current one): packed words, where they begin, the seed's offset in its read, the read's length
    SeedWords W = { 0, 0, 0, 0, 0 }; uint32_t w_begin = 0, w_pfw = 0, w_rlen = 0; bool w_valid = false;
    // stage 2 -> 3 (the current tile): seed bits, table entry, orientation
    uint64_t V = 0; uint4 e = make_uint4( 1u, 0u, 0u, 0u ); bool e_valid = false; uint32_t qo = 0, c_pfw = 0, c_rlen = 0; bool c_seed = false;
    {
        const uint32_t rid = tile * tl.rpt + lr;
        if (lane_ok && rid < tl.reads)
        {
            uint32_t b0;
            c_seed = seed_geom( rid, b0, c_pfw, c_rlen );
            if (c_seed)
            {
                const SeedWords W0 = load_seed_words<BITS>( q.symbols, b0, len );
                e_valid = seed_bits_from_words<BITS>( W0, b0, len, false, false, V );
                if (e_valid) e = entry_of( V, qo );
            }
        }
        const uint32_t t1 = tile + n_waves, rid1 = t1 * tl.rpt + lr;
        if (t1 < tl.n_tiles && lane_ok && rid1 < tl.reads)
        {
            w_valid = seed_geom( rid1, w_begin, w_pfw, w_rlen );
            if (w_valid) W = load_seed_words<BITS>( q.symbols, w_begin, len );
        }
    }
    for (; tile < tl.n_tiles; tile += n_waves)
    {
        const uint32_t rid = tile * tl.rpt + lr;
        const bool valid = lane_ok && rid < tl.reads && c_seed;
        // ---- stage 3a: the kind of entry; the group of a k-mer with 2..8 occurrences is requested ----
        const bool is_one   = e_valid && e.y >= DTAB_MARK && e.x < DTAB_MARK;
        const bool is_group = e_valid && e.y >= DTAB_MARK && e.x >= DTAB_MARK;
        const bool is_heavy = e_valid && e.y < DTAB_MARK && e.x <= e.y;
        uint4 q0 = make_uint4( 0, 0, 0, 0 ), q1 = q0, q2 = q0, q3 = q0;
        const uint32_t m = e.y - DTAB_MARK;
        if (is_group)
        {
            const uint4* g4 = (const uint4*)(f.cside + 4ull * (e.x - DTAB_MARK));
            q0 = g4[0]; q1 = g4[1];
            if (m > 4u) { q2 = g4[2]; q3 = g4[3]; }
        }
        // ---- stage 2 for the next tile ----
        uint64_t Vn = 0; uint4 en = make_uint4( 1u, 0u, 0u, 0u ); bool en_valid = false; uint32_t qon = 0;
        const uint32_t n_pfw = w_pfw, n_rlen = w_rlen; const bool n_seed = w_valid;
        if (w_valid)
        {
            en_valid = seed_bits_from_words<BITS>( W, w_begin, len, false, false, Vn );
            if (en_valid) en = entry_of( Vn, qon );
        }
        // ---- stage 1 for the tile after next ----
        {
            const uint32_t t2 = tile + 2u * n_waves, rid2 = t2 * tl.rpt + lr;
            w_valid = t2 < tl.n_tiles && lane_ok && rid2 < tl.reads;
            if (w_valid) w_valid = seed_geom( rid2, w_begin, w_pfw, w_rlen );
            if (w_valid) W = load_seed_words<BITS>( q.symbols, w_begin, len );
        }
        // ---- stage 3b: resolve the current tile ----
        resolve_tile( tile, rid, valid, V, e, e_valid, qo, c_pfw, c_rlen, is_one, is_group, is_heavy, q0, q1, q2, q3, 0u, 0u );
        V = Vn; e = en; e_valid = en_valid; qo = qon; c_pfw = n_pfw; c_rlen = n_rlen; c_seed = n_seed;
    }
}

// The deferred searches of fm_seed_both_kernel<.., DEFER = true> as a dense launch: entry t of `list` (n = *n_list) is
// (seed id | strand << 31); the ordinary search of that strand (plain table + rank steps + finish on the text) ends on
//   one text occurrence       -> its diagonal key, appended behind the compacted keys (keys_out + counts[0], counts[0] advanced)
//   several rows (a repeat)   -> that strand's residual list (counts[1 + strand]), as the in-line search would
//   nothing                   -> nothing.
// Every lane runs four searches, then the workgroup appends what they left with ONE returning atomic per output list (a wave-level
// append per list would put 2 x 10^5 atomics on two neighbouring words for 9 M searches: at ~11 ns each, longer than the searches).
constexpr uint32_t HEAVY_PER_LANE = 4u;
template <int BITS>
__global__ void __launch_bounds__(256)
fm_seed_heavy_kernel(const DevIndex f, const StringSetDev q, const uint32_t read_len, const uint32_t* __restrict__ list, const uint32_t* __restrict__ n_list,
                     uint64_t* __restrict__ keys_out, uint2* __restrict__ res_ranges, uint32_t* __restrict__ res_ids, const uint32_t res_cap,
                     unsigned int* __restrict__ counts)
{
    __shared__ uint32_t s_cnt[4][3], s_base[3];
    const uint32_t n = *n_list;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t len = q.fixed_len;
    const bool ragged = q.intervals != nullptr;
    DevIndex fplain = f; fplain.dtab = nullptr; fplain.dkmer = 0;
    const uint32_t chunk = 256u * HEAVY_PER_LANE;
    for (uint32_t c0 = blockIdx.x * chunk; c0 < n; c0 += gridDim.x * chunk)           // (block-uniform trip count: the barriers below are safe)
    {
        uint32_t kind[HEAVY_PER_LANE], vx[HEAVY_PER_LANE], vy[HEAVY_PER_LANE], ent[HEAVY_PER_LANE];
        uint32_t nk = 0, nr0 = 0, nr1 = 0;                                            // this lane's keys / forward residuals / reverse residuals
        #pragma unroll
        for (uint32_t u = 0; u < HEAVY_PER_LANE; ++u)
        {
            const uint32_t t = c0 + u * 256u + threadIdx.x;
            kind[u] = 0u; vx[u] = 1u; vy[u] = 0u; ent[u] = 0u;
            if (t < n)
            {
                ent[u] = list[t];
                const uint32_t i = ent[u] & 0x7FFFFFFFu, s = ent[u] >> 31;
                uint32_t rx, ry, nblk; bool single;
                match_one<BITS,false,true,true>( fplain, q, s ? (NVBIO_FM_SCAN_FORWARD | NVBIO_FM_COMPLEMENT) : 0u, f.ktab != nullptr, false, i, rx, ry, nblk, single );
                if (!single && rx == ry) { const uint32_t sv = f.ssa[rx]; rx = ry = (sv == 0xFFFFFFFFu) ? f.length : sv; single = true; }
                if (single)        { kind[u] = 1u; vx[u] = rx; ++nk; }
                else if (rx < ry)  { kind[u] = 2u + s; vx[u] = rx; vy[u] = ry; if (s) ++nr1; else ++nr0; }
            }
        }
        // exclusive prefix of the three counts within the wave, wave totals to LDS, one atomic per list and workgroup
        uint32_t pk = nk, p0 = nr0, p1 = nr1;
        #pragma unroll
        for (int d = 1; d < 64; d <<= 1)
        {
            const uint32_t a = (uint32_t)__shfl_up( (int)pk, d ), b = (uint32_t)__shfl_up( (int)p0, d ), c = (uint32_t)__shfl_up( (int)p1, d );
            if (lane >= (uint32_t)d) { pk += a; p0 += b; p1 += c; }
        }
        if (lane == 63u) { s_cnt[wave][0] = pk; s_cnt[wave][1] = p0; s_cnt[wave][2] = p1; }
        __syncthreads();
        if (threadIdx.x < 3u)
        {
            const uint32_t tot = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
            s_base[threadIdx.x] = tot ? atomicAdd( &counts[threadIdx.x], tot ) : 0u;
        }
        __syncthreads();
        uint32_t ok = s_base[0] + (pk - nk), o0 = s_base[1] + (p0 - nr0), o1 = s_base[2] + (p1 - nr1);
        for (uint32_t w = 0; w < wave; ++w) { ok += s_cnt[w][0]; o0 += s_cnt[w][1]; o1 += s_cnt[w][2]; }
        #pragma unroll
        for (uint32_t u = 0; u < HEAVY_PER_LANE; ++u)
        {
            const uint32_t i = ent[u] & 0x7FFFFFFFu, s = ent[u] >> 31;
            if (kind[u] == 1u)
            {
                const uint32_t rid = i / q.spr, j = i - rid * q.spr;
                uint32_t pq = j * (ragged ? q.intervals[rid] : q.interval);
                const uint32_t rlen = ragged ? q.offsets[rid + 1] - q.offsets[rid] : read_len;
                if (s) pq = rlen - pq - len;
                keys_out[ok++] = ((uint64_t)rid << 34) | ((uint64_t)s << 33) | ((uint64_t)vx[u] + 1024u - pq);
            }
            else if (kind[u] == 2u) { res_ranges[o0] = make_uint2( vx[u], vy[u] ); res_ids[o0] = i; ++o0; }
            else if (kind[u] == 3u) { res_ranges[res_cap + o1] = make_uint2( vx[u], vy[u] ); res_ids[res_cap + o1] = i; ++o1; }
        }
        __syncthreads();                                                              // s_cnt / s_base are reused by the next chunk
    }
}

// the deferred slots of every tile made dense (as fm_seed_compact_kernel does with the keys); counts_out[0] = their number
__global__ void __launch_bounds__(256)
fm_seed_defer_compact_kernel(const uint32_t* __restrict__ tile_defer, const uint32_t* __restrict__ defer_counts, const uint32_t* __restrict__ defer_offsets,
                             const uint32_t n_tiles, uint32_t* __restrict__ list, uint32_t* __restrict__ n_out)
{
    for (uint32_t tile = blockIdx.x * blockDim.x + threadIdx.x; tile < n_tiles; tile += gridDim.x * blockDim.x)
    {
        const uint32_t n = defer_counts[tile], off = defer_offsets[tile];
        const uint32_t* src = tile_defer + (uint64_t)tile * 128u;
        for (uint32_t k = 0; k < n; ++k) list[off + k] = src[k];
        if (tile == n_tiles - 1u) n_out[0] = off + n;
    }
}
