// common.h -- shared host/device helpers of the MI355X seed-and-extend core (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <type_traits>
#include <vector>

#include "../../include/nvbio_amd.h"

namespace nvbio_amd {

// ---- error handling: status codes + a thread-local message, never exceptions ----------------
void        set_error(const char* fmt, ...);
const char* get_error();

#define NVB_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            nvbio_amd::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
            return NVBIO_ERR_HIP;                                                                  \
        }                                                                                          \
    } while (0)

#define NVB_CHECK(call)                                                                            \
    do { nvbio_status _s = (call); if (_s != NVBIO_OK) return _s; } while (0)

#define NVB_REQUIRE(cond, msg)                                                                     \
    do { if (!(cond)) { nvbio_amd::set_error("invalid argument: %s", msg); return NVBIO_ERR_INVALID; } } while (0)

// the calls that form diagonal keys (read << 34 | strand << 33 | diagonal + 1024): see NVBIO_MAX_SEED_OFFSET in nvbio_amd.h
#define NVB_SEED_OFFSET_MSG "read_len - seed_len exceeds 1024 (NVBIO_MAX_SEED_OFFSET): a diagonal could leave the key's 33-bit field"

// Scratch with stream-ordered semantics WITHOUT the runtime's stream-ordered pool: a block taken by a ScratchBlock may be used by work enqueued on
// `s` after the call; the ScratchBlock's destruction gives it back at once, for the next call on the SAME stream (whose work runs behind everything
// that used the block).  Blocks are plain hipMalloc allocations cached per (device, stream).  Why not hipMallocAsync / hipFreeAsync: on ROCm 7.2 a
// block RE-used from the default pool did not hold what a kernel had just written into it -- the flags of the banded scorer's first pass read back as
// zeros in the second call of a process (seen with hipMemcpy right behind the kernel; with hipMalloc / hipFree in its place: never).  A few fresh-box
// runs also scored 61,818 reads of 10 M -20 instead of -18 in production; that those read zeros from a pool block is inferred, not observed.  What
// is established: under the scratch check mode below (exact-size guard-banded blocks filled with 0x00, 0xFF or 0x02) every site's parity cases
// equal the oracle and no band or gap is touched (tests/test_gpu_scratch_check.py), so no library kernel overruns its scratch or reads scratch it
// did not write at the tested shapes; and a cached block that still holds the previous batch's flags gives the oracle's results.  core.hip.
void scratch_release_idle();                              // hipFree every idle block (each behind a synchronisation of its stream)

// Scratch check mode (nvbio_amd_set_scratch_check, a test tool, off by default): every ScratchBlock takes a fresh exact-size hipMalloc with a
// guard band at each end, the layouts leave a gap before each sub-array and after the last, blocks (a caller's temp included) and BuildBuffers are
// filled with one byte before any work, and each block's bands and gaps are read back when it is given back.  core.hip.
bool    scratch_check_enabled();
uint8_t scratch_check_fill();

// The sub-arrays of one scratch block in order, declared once per site by code that runs twice: over ScratchLayout() it only adds up their
// sizes, over ScratchLayout( block ) it also hands out their pointers.  Every sub-array starts on a 256-byte boundary (hipcub temporaries need that).
// With `check` (check mode, read once per block) every sub-array is preceded by a gap of 256 bytes and the last one followed by one; `extents`,
// when given, receives each sub-array's [begin, end) in the block.
class ScratchLayout
{
public:
    static const uint64_t GAP = 256u;
    explicit ScratchLayout(uint8_t* base = nullptr, bool check = false, std::vector<uint64_t>* extents = nullptr)
        : base_( base ), check_( check ), extents_( extents ) {}
    template <typename T> T* take(uint64_t count)
    {
        const uint64_t at = round( end_ ) + (check_ ? GAP : 0u);
        end_ = at + count * sizeof(T);
        if (extents_) { extents_->push_back( at ); extents_->push_back( end_ ); }
        return base_ ? (T*)(base_ + at) : nullptr;
    }
    uint64_t end() const   { return check_ ? round( end_ ) + GAP : end_; }   // the bytes a block must hold
    uint64_t bytes() const { return round( end() ) + 256u; }               // the bytes a caller's buffer must hold: room to align its start
    static uint64_t round(uint64_t x) { return (x + 255u) & ~255ull; }
private:
    uint8_t* base_;
    bool     check_;
    std::vector<uint64_t>* extents_;
    uint64_t end_ = 0;
};

struct ScratchCheckState;                                  // the check-mode bookkeeping of one block (core.hip)

// The scratch of one call: a block of the cache above for stream `s` (alloc), or the caller's temp_dev (adopt).  Only a block it took from the
// cache is given back, when it goes out of scope -- so every exit of the call gives it back.  `tag` names the site in the check-mode report.
class ScratchBlock
{
public:
    ScratchBlock() = default;
    ScratchBlock(ScratchBlock&& o) noexcept : p_( o.p_ ), s_( o.s_ ), own_( o.own_ ), chk_( o.chk_ ) { o.p_ = nullptr; o.own_ = false; o.chk_ = nullptr; }
    ScratchBlock& operator=(ScratchBlock&& o) noexcept
    {
        if (this != &o) { release(); p_ = o.p_; s_ = o.s_; own_ = o.own_; chk_ = o.chk_; o.p_ = nullptr; o.own_ = false; o.chk_ = nullptr; }
        return *this;
    }
    ScratchBlock(const ScratchBlock&) = delete;
    ScratchBlock& operator=(const ScratchBlock&) = delete;
    ~ScratchBlock() { release(); }

    // `bytes` of the cache for work on `s`; out of memory: the message printf( fmt, ... ) and NVBIO_ERR_NOMEM
    nvbio_status alloc(const char* tag, uint64_t bytes, hipStream_t s, const char* fmt, ...);
    // the block for the sub-arrays that layout( ScratchLayout& ) declares, run once to size it and once to set the site's pointers into it:
    // alloc (msg: a format given the block's bytes as unsigned long long), or adopt when the caller passes its temp (sized by `query`);
    // `at`: the block starts that many bytes, rounded up to 256, into the caller's temp (behind another block of the same call)
    template <typename Layout>
    nvbio_status alloc_layout(const char* tag, hipStream_t s, const char* msg, Layout layout, void* temp = nullptr, uint64_t temp_bytes = 0,
                              const char* query = nullptr, uint64_t at = 0)
    {
        const bool check = scratch_check_enabled();
        ScratchLayout size( nullptr, check ); layout( size );
        NVB_CHECK( temp ? adopt( tag, temp, temp_bytes, at, size.end(), query, s, check )
                        : alloc_impl( tag, size.end(), s, check, msg, (unsigned long long)size.end() ) );
        ScratchLayout c( p_, check, check ? extents() : nullptr ); layout( c );
        return NVBIO_OK;
    }
    uint8_t* get() const { return p_; }

private:
    nvbio_status alloc_impl(const char* tag, uint64_t bytes, hipStream_t s, bool check, const char* fmt, ...);
    nvbio_status alloc_v(const char* tag, uint64_t bytes, hipStream_t s, bool check, const char* fmt, va_list ap);
    // `bytes` of the caller's `temp_bytes` at `temp`, from round( at ) on behind its start aligned up to 256: else NVBIO_ERR_INVALID and
    // "temp_bytes <temp_bytes> too small: this call needs <n> (<query>)", n = ScratchLayout::bytes() of a buffer that ends with this block
    nvbio_status adopt(const char* tag, void* temp, uint64_t temp_bytes, uint64_t at, uint64_t bytes, const char* query, hipStream_t s, bool check);
    std::vector<uint64_t>* extents();                      // check mode: the sub-array extents the pointer pass records
    void release();
    uint8_t*    p_   = nullptr;
    hipStream_t s_   = nullptr;
    bool        own_ = false;
    ScratchCheckState* chk_ = nullptr;                     // check mode only
};

// RAII for the hipMalloc temporaries of an index build (not the stream scratch above): every buffer it allocated and was not told to
// forget (ownership handed over) is freed when it goes out of scope.  In check mode each buffer is filled (no guard bands) before it is handed out.
// `what` names the build in NVB_ALLOC's out-of-memory message.  It counts the bytes it holds (`live`) and the most it ever held (`peak`).
struct BuildBuffers
{
    std::vector<void*>  ptrs;
    std::vector<size_t> sizes;                                // of ptrs, in order
    uint64_t            live = 0, peak = 0;
    const char*         what;
    explicit BuildBuffers(const char* what = "index build") : what( what ) {}
    ~BuildBuffers() { for (void* p : ptrs) (void)hipFree( p ); }
    template <typename T> T* alloc(size_t count)            // nullptr when out of memory
    {
        void* p = nullptr;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        if (hipMalloc( &p, bytes ) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        ptrs.push_back( p ); sizes.push_back( bytes );
        live += bytes; if (live > peak) peak = live;
        if (scratch_check_enabled() && (hipMemset( p, scratch_check_fill(), bytes ) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
        {
            (void)hipGetLastError(); return nullptr;
        }
        return (T*)p;
    }
    void release(void* p) { if (drop( p )) (void)hipFree( p ); }
    void forget(void* p)  { (void)drop( p ); }
private:
    bool drop(void* p)
    {
        for (size_t i = 0; i < ptrs.size(); ++i)
            if (ptrs[i] == p) { live -= sizes[i]; ptrs.erase( ptrs.begin() + i ); sizes.erase( sizes.begin() + i ); return true; }
        return false;
    }
};

// T* var = `count` T's of the BuildBuffers `bufs` in scope; out of memory: "<bufs.what>: out of device memory (var, <bytes> bytes)" and
// NVBIO_ERR_NOMEM
#define NVB_ALLOC(var, T, count)                                                                   \
    T* var = bufs.alloc<T>( count );                                                               \
    if (!var) { nvbio_amd::set_error( "%s: out of device memory (%s, %zu bytes)", bufs.what, #var, (size_t)(count) * sizeof(T) ); return NVBIO_ERR_NOMEM; }

// ---- runtime value -> template argument ------------------------------------------------------
// Values<...> lists the values a template is instantiated for, BitsList<Bits<r, t>, ...> the (read_bits, text_bits) pairs.
// with_value( list, v, f, miss ) returns f( std::integral_constant<int, V>() ) for the listed V equal to v, with_bits( list, rbits,
// tbits, f, miss ) returns f( Bits<r, t>() ) for the listed pair equal to (rbits, tbits); either returns miss() when the list holds no
// such entry, so that each call site keeps its own status and message.  Every entry instantiates f; the choice is a chain of compares.
template <int... Vs> struct Values {};
using SymbolBits = Values<2, 4, 8>;                       // the symbol widths of an nvbio_string_set: kernels over strings are instantiated for each
nvbio_status bad_symbol_bits();                           // the miss of a dispatch over SymbolBits: "symbol_bits must be 2, 4 or 8", NVBIO_ERR_INVALID
template <int R, int T> struct Bits { static constexpr int r = R, t = T; };
template <typename... Ps> struct BitsList {};

template <int... Vs, typename F, typename Miss>
inline auto with_value(Values<Vs...>, const int v, F&& f, Miss&& miss) -> decltype(miss())
{
    decltype(miss()) r{};
    return ((v == Vs && ((r = f( std::integral_constant<int, Vs>() )), true)) || ...) ? r : miss();
}
template <typename... Ps, typename F, typename Miss>
inline auto with_bits(BitsList<Ps...>, const uint32_t rbits, const uint32_t tbits, F&& f, Miss&& miss) -> decltype(miss())
{
    decltype(miss()) r{};
    return ((rbits == (uint32_t)Ps::r && tbits == (uint32_t)Ps::t && ((r = f( Ps() )), true)) || ...) ? r : miss();
}

// select the device and fail loudly if it is not a gfx950: there is no CPU fallback
nvbio_status use_device(int device);

// RAII device switch that restores the caller's current device
struct DeviceGuard
{
    int  prev;
    bool ok;
    explicit DeviceGuard(int device) : prev(-1), ok(false)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (use_device(device) == NVBIO_OK);
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// launch-grid helper: enough 256-thread workgroups for n items, capped so that the grid stays
// a small multiple of the chip (256 CUs x 8 blocks) and the kernels grid-stride the rest
static inline unsigned grid_for(uint64_t n, unsigned block = 256, unsigned cap_blocks = 256u * 32u)
{
    uint64_t b = (n + block - 1) / block;
    if (b < 1) b = 1;
    if (b > cap_blocks) b = cap_blocks;
    return (unsigned)b;
}

// ---- kernel launch ---------------------------------------------------------------------------
// Every kernel of the library is launched here, and every launch is checked: NVB_LAUNCH( kernel, grid, block, stream, args... )
// enqueues the kernel (none takes dynamic LDS) and returns NVBIO_OK, or NVBIO_ERR_HIP and the message "<kernel> launch failed:
// <the runtime's reason>" when the runtime rejects the launch -- so a bad launch is reported by its own site, under its own name.
// A call site wraps it in NVB_CHECK, or keeps the status where it carries one through a loop.  A kernel whose template arguments
// hold a comma goes in parentheses.  The arguments convert to the kernel's parameter types as in a plain call.
template <typename... P, typename... A>
inline nvbio_status launch_kernel(const char* what, void (*kernel)(P...), const dim3 grid, const dim3 block, hipStream_t s, A&&... args)
{
    hipLaunchKernelGGL( kernel, grid, block, 0, s, args... );
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error( "%s launch failed: %s", what, hipGetErrorString( e ) ); return NVBIO_ERR_HIP; }
    return NVBIO_OK;
}
#define NVB_LAUNCH(kernel, ...) nvbio_amd::launch_kernel( #kernel, kernel, __VA_ARGS__ )

// ---- device-side symbol access --------------------------------------------------------------
// Big-endian packed streams (PackedStream<..,BITS,true>): symbol i of a 2-bit stream sits at bits
// [30-2(i&15), 31-2(i&15)] of word i>>4; of a 4-bit stream at [28-4(i&7), 31-4(i&7)] of word i>>3.
// The reader keeps the last word in a register so that a scan over consecutive symbols issues
// one load per 16 (8) symbols.
template <int BITS>
struct SymbolReader
{
    const uint32_t* words;
    uint32_t        cur_idx;
    uint32_t        cur;
    __device__ __forceinline__ explicit SymbolReader(const void* p) : words((const uint32_t*)p), cur_idx(0xFFFFFFFFu), cur(0) {}
    __device__ __forceinline__ uint32_t get(uint32_t i)
    {
        constexpr uint32_t LOG = (BITS == 2) ? 4 : 3;
        constexpr uint32_t PER = 1u << LOG;
        const uint32_t w = i >> LOG;
        if (w != cur_idx) { cur = words[w]; cur_idx = w; }
        return (cur >> ((32u - BITS) - BITS * (i & (PER - 1u)))) & ((1u << BITS) - 1u);
    }
};
template <>
struct SymbolReader<8>
{
    const uint8_t* bytes;
    __device__ __forceinline__ explicit SymbolReader(const void* p) : bytes((const uint8_t*)p) {}
    __device__ __forceinline__ uint32_t get(uint32_t i) { return bytes[i]; }
};

} // namespace nvbio_amd
