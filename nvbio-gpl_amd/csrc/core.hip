// core.hip -- status/error plumbing and device selection of the C ABI.
#include "common.h"
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

namespace nvbio_amd {

static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start( ap, fmt );
    vsnprintf( g_error, sizeof(g_error), fmt, ap );
    va_end( ap );
}
const char* get_error() { return g_error; }

nvbio_status bad_symbol_bits() { set_error( "invalid argument: symbol_bits must be 2, 4 or 8" ); return NVBIO_ERR_INVALID; }

// ---- scratch blocks cached per (device, stream): see common.h ----
namespace {
struct CachedBlock { void* p; size_t cap; bool busy; int device; hipStream_t stream; };
std::mutex                 g_scratch_mutex;
std::vector<CachedBlock>   g_scratch;
const size_t SCRATCH_KEEP_PER_STREAM = 32ull << 30;             // idle blocks beyond this are released (after the stream has drained)

// hipFree the idle blocks `match` selects, each behind a synchronisation of its own stream (work behind which the block was given back may still
// use it); the caller holds the mutex
template <typename Match>
void release_idle(Match match)
{
    int prev = -1; (void)hipGetDevice( &prev );
    for (size_t i = 0; i < g_scratch.size(); )
    {
        const CachedBlock& b = g_scratch[i];
        if (!b.busy && match( b ))
        {
            (void)hipSetDevice( b.device );
            (void)hipStreamSynchronize( b.stream );
            (void)hipFree( b.p );
            g_scratch.erase( g_scratch.begin() + i );
        }
        else ++i;
    }
    if (prev >= 0) (void)hipSetDevice( prev );
}

hipError_t scratch_alloc(void** p, size_t bytes, hipStream_t s)
{
    *p = nullptr;
    int dev = 0;
    hipError_t e = hipGetDevice( &dev );
    if (e != hipSuccess) return e;
    if (bytes == 0) bytes = 256;
    const size_t want = (bytes + ((2u << 20) - 1u)) & ~(size_t)((2u << 20) - 1u);
    std::lock_guard<std::mutex> lock( g_scratch_mutex );
    // best fit among this stream's idle blocks (any larger block will do: a loop whose requests shrink from pass to pass must not allocate in every pass)
    int best = -1;
    for (size_t i = 0; i < g_scratch.size(); ++i)
    {
        const CachedBlock& b = g_scratch[i];
        if (!b.busy && b.device == dev && b.stream == s && b.cap >= want && (best < 0 || b.cap < g_scratch[best].cap)) best = (int)i;
    }
    if (best >= 0) { g_scratch[best].busy = true; *p = g_scratch[best].p; return hipSuccess; }
    void* q = nullptr;
    e = hipMalloc( &q, want );
    if (e != hipSuccess)
    {
        // out of memory: give every idle block of the device back (of any stream, each once its stream has drained) and try once more
        (void)hipGetLastError();
        release_idle( [dev](const CachedBlock& b) { return b.device == dev; } );
        e = hipMalloc( &q, want );
        if (e != hipSuccess) return e;
    }
    g_scratch.push_back( CachedBlock{ q, want, true, dev, s } );
    *p = q;
    return hipSuccess;
}

void scratch_free(void* p, hipStream_t s)
{
    std::lock_guard<std::mutex> lock( g_scratch_mutex );
    size_t idle = 0; int dev = -1;
    for (CachedBlock& b : g_scratch)
        if (b.p == p) { b.busy = false; dev = b.device; }
    for (const CachedBlock& b : g_scratch) if (!b.busy && b.device == dev && b.stream == s) idle += b.cap;
    if (idle > SCRATCH_KEEP_PER_STREAM)
        release_idle( [dev, s](const CachedBlock& b) { return b.device == dev && b.stream == s; } );
}
}

void scratch_release_idle()
{
    std::lock_guard<std::mutex> lock( g_scratch_mutex );
    release_idle( [](const CachedBlock&) { return true; } );
}

// ---- scratch check mode: see common.h ----
struct ScratchCheckState
{
    const char*           tag;
    uint8_t*              base;         // what check mode hipMalloc'ed (nullptr: the caller's temp)
    int64_t               lo, hi;       // the checked span around p_: [p_ + lo, p_ + hi)
    std::vector<uint64_t> extents;      // the sub-arrays' [begin, end) pairs
};

namespace {
struct CheckRecord { uint64_t checked = 0, damaged = 0; int64_t first_sub = -1, first_off = 0; };
std::atomic<bool>                  g_check_on{ false };
uint8_t                            g_check_fill = 0;
std::mutex                         g_check_mutex;
std::vector<std::pair<std::string, CheckRecord>> g_check_report;    // in the order the sites were first seen
const int64_t CHECK_BAND = 4096;                                     // guard band at each end of a block check mode allocates

CheckRecord& check_record(const char* tag)
{
    for (auto& r : g_check_report) if (r.first == tag) return r.second;
    g_check_report.emplace_back( tag, CheckRecord() );
    return g_check_report.back().second;
}
}

bool    scratch_check_enabled() { return g_check_on.load( std::memory_order_relaxed ); }
uint8_t scratch_check_fill()    { return g_check_fill; }

nvbio_status ScratchBlock::alloc(const char* tag, uint64_t bytes, hipStream_t s, const char* fmt, ...)
{
    va_list ap;
    va_start( ap, fmt );
    const nvbio_status st = alloc_v( tag, bytes, s, scratch_check_enabled(), fmt, ap );
    va_end( ap );
    return st;
}

nvbio_status ScratchBlock::alloc_impl(const char* tag, uint64_t bytes, hipStream_t s, bool check, const char* fmt, ...)
{
    va_list ap;
    va_start( ap, fmt );
    const nvbio_status st = alloc_v( tag, bytes, s, check, fmt, ap );
    va_end( ap );
    return st;
}

nvbio_status ScratchBlock::alloc_v(const char* tag, uint64_t bytes, hipStream_t s, bool check, const char* fmt, va_list ap)
{
    release();
    if (check)
    {
        // a fresh exact-size block between two guard bands, all of it filled before any work of the call
        void* p = nullptr;
        if (hipMalloc( &p, bytes + 2 * CHECK_BAND ) != hipSuccess)
        {
            (void)hipGetLastError();
            vsnprintf( g_error, sizeof(g_error), fmt, ap );
            return NVBIO_ERR_NOMEM;
        }
        chk_ = new ScratchCheckState{ tag, (uint8_t*)p, -CHECK_BAND, (int64_t)bytes + CHECK_BAND, { 0, bytes } };
        p_ = (uint8_t*)p + CHECK_BAND; s_ = s; own_ = false;
        NVB_HIP( hipMemsetAsync( p, g_check_fill, bytes + 2 * CHECK_BAND, s ) );
        return NVBIO_OK;
    }
    void* p = nullptr;
    if (scratch_alloc( &p, bytes, s ) != hipSuccess)
    {
        (void)hipGetLastError();
        vsnprintf( g_error, sizeof(g_error), fmt, ap );
        return NVBIO_ERR_NOMEM;
    }
    p_ = (uint8_t*)p; s_ = s; own_ = true;
    return NVBIO_OK;
}

nvbio_status ScratchBlock::adopt(const char* tag, void* temp, uint64_t temp_bytes, uint64_t at, uint64_t bytes, const char* query, hipStream_t s, bool check)
{
    release();
    const uint64_t skip = (256u - ((uintptr_t)temp & 255u)) & 255u;
    at = ScratchLayout::round( at );
    if (temp == nullptr || temp_bytes < skip || temp_bytes - skip < at + bytes)
    {
        set_error( "invalid argument: temp_bytes %llu too small: this call needs %llu (%s)", (unsigned long long)temp_bytes,
                   (unsigned long long)(ScratchLayout::round( at + bytes ) + 256u), query );
        return NVBIO_ERR_INVALID;
    }
    p_ = (uint8_t*)temp + skip + at;
    if (check)
    {
        // the caller's buffer from the block's start on is filled (the first block's from the buffer's start); checked: the alignment skip
        // (the first block's), the gaps and at most a band's worth behind the layout
        const uint64_t lead = at ? 0u : skip, tail = temp_bytes - skip - at - bytes;
        chk_ = new ScratchCheckState{ tag, nullptr, -(int64_t)lead, (int64_t)(bytes + (tail < (uint64_t)CHECK_BAND ? tail : (uint64_t)CHECK_BAND)), { 0, bytes } };
        s_ = s;
        NVB_HIP( hipMemsetAsync( p_ - lead, g_check_fill, lead + bytes + tail, s ) );
    }
    return NVBIO_OK;
}

std::vector<uint64_t>* ScratchBlock::extents()
{
    if (!chk_) return nullptr;
    chk_->extents.clear();                                  // the layout's sub-arrays replace the whole-block extent
    return &chk_->extents;
}

void ScratchBlock::release()
{
    if (own_) scratch_free( p_, s_ );
    if (chk_)
    {
        // check mode: once the call's work has drained, every byte of the bands and gaps must still hold the fill
        ScratchCheckState& c = *chk_;
        if (hipStreamSynchronize( s_ ) == hipSuccess)
        {
            bool bad = false; int64_t bad_sub = -1, bad_off = 0;
            std::vector<uint8_t> h;
            int64_t from = c.lo;
            const size_t n = c.extents.size() / 2;
            for (size_t i = 0; i <= n && !bad; ++i)
            {
                const int64_t to = i < n ? (int64_t)c.extents[2 * i] : c.hi;            // the gap behind sub-array i - 1
                if (to > from)
                {
                    h.resize( (size_t)(to - from) );
                    if (hipMemcpy( h.data(), p_ + from, h.size(), hipMemcpyDeviceToHost ) != hipSuccess) { (void)hipGetLastError(); break; }
                    for (size_t k = 0; k < h.size(); ++k)
                        if (h[k] != g_check_fill) { bad = true; bad_sub = (int64_t)i - 1; bad_off = from + (int64_t)k; break; }
                }
                if (i < n) from = (int64_t)c.extents[2 * i + 1];
            }
            std::lock_guard<std::mutex> lock( g_check_mutex );
            CheckRecord& r = check_record( c.tag );
            ++r.checked;
            if (bad && r.damaged++ == 0) { r.first_sub = bad_sub; r.first_off = bad_off; }
        }
        else (void)hipGetLastError();
        if (c.base) (void)hipFree( c.base );
        delete chk_; chk_ = nullptr;
    }
    p_ = nullptr; own_ = false;
}

nvbio_status use_device(int device)
{
    int count = 0;
    if (hipGetDeviceCount( &count ) != hipSuccess || count <= 0)
    {
        set_error( "no HIP device is visible: this library has no CPU fallback" );
        return NVBIO_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count)
    {
        set_error( "device %d out of range (%d visible)", device, count );
        return NVBIO_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties( &prop, device ) != hipSuccess)
    {
        set_error( "hipGetDeviceProperties(%d) failed", device );
        return NVBIO_ERR_HIP;
    }
    if (strncmp( prop.gcnArchName, "gfx950", 6 ) != 0)
    {
        set_error( "device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName );
        return NVBIO_ERR_NO_DEVICE;
    }
    if (hipSetDevice( device ) != hipSuccess)
    {
        set_error( "hipSetDevice(%d) failed", device );
        return NVBIO_ERR_HIP;
    }
    // (scratch -- boundary columns, direction vectors, scan temporaries -- comes from the ScratchBlock cache above, not from the runtime's stream-ordered pool)
    return NVBIO_OK;
}

} // namespace nvbio_amd

using namespace nvbio_amd;

extern "C" {

int         nvbio_amd_version(void)    { return NVBIO_AMD_VERSION; }
nvbio_status nvbio_amd_release_scratch(void) { scratch_release_idle(); return NVBIO_OK; }
const char* nvbio_amd_last_error(void) { return get_error(); }

nvbio_status nvbio_amd_set_scratch_check(int enable, uint32_t fill_byte)
{
    NVB_REQUIRE( fill_byte <= 0xFFu, "fill_byte must be a byte" );
    std::lock_guard<std::mutex> lock( g_check_mutex );
    if (enable) { g_check_report.clear(); g_check_fill = (uint8_t)fill_byte; }
    g_check_on.store( enable != 0 );
    return NVBIO_OK;
}

nvbio_status nvbio_amd_scratch_check_report(char* buf, uint64_t buf_len)
{
    NVB_REQUIRE( buf != nullptr && buf_len > 0, "buf is NULL" );
    std::lock_guard<std::mutex> lock( g_check_mutex );
    std::string out;
    char line[256];
    for (const auto& r : g_check_report)
    {
        if (r.second.damaged) snprintf( line, sizeof(line), "%s %llu %llu %lld %lld\n", r.first.c_str(), (unsigned long long)r.second.checked,
                                        (unsigned long long)r.second.damaged, (long long)r.second.first_sub, (long long)r.second.first_off );
        else                  snprintf( line, sizeof(line), "%s %llu 0 - -\n", r.first.c_str(), (unsigned long long)r.second.checked );
        out += line;
    }
    NVB_REQUIRE( out.size() < buf_len, "buf_len too small for the report" );
    memcpy( buf, out.c_str(), out.size() + 1 );
    return NVBIO_OK;
}

nvbio_status nvbio_amd_device_count(int* count)
{
    NVB_REQUIRE( count != nullptr, "count is NULL" );
    *count = 0;
    if (hipGetDeviceCount( count ) != hipSuccess) { *count = 0; set_error( "hipGetDeviceCount failed" ); return NVBIO_ERR_NO_DEVICE; }
    return NVBIO_OK;
}

nvbio_status nvbio_amd_device_arch(int device, char* name, uint32_t name_len)
{
    NVB_REQUIRE( name != nullptr && name_len > 0, "name buffer is NULL" );
    hipDeviceProp_t prop;
    NVB_HIP( hipGetDeviceProperties( &prop, device ) );
    strncpy( name, prop.gcnArchName, name_len - 1 );
    name[name_len - 1] = 0;
    return NVBIO_OK;
}

nvbio_status nvbio_amd_stream_synchronize(int device, void* stream)
{
    DeviceGuard g( device ); if (!g.ok) return NVBIO_ERR_NO_DEVICE;
    NVB_HIP( hipStreamSynchronize( (hipStream_t)stream ) );
    return NVBIO_OK;
}

} // extern "C"
