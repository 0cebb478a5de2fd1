/*
 * oracle/refshim/refshim_launch.h -- runs a kernel over a grid and a block on the host.
 * TEST INFRASTRUCTURE ONLY (see cuda_runtime.h).
 *
 *   refshim::run(grid, block, shared, body)          blocks and threads as plain loops; a
 *                                                    __syncthreads() in the body is an error
 *   refshim::run_threads(grid, block, shared, body)  one host thread per GPU thread of a block,
 *                                                    __syncthreads() is a real barrier that
 *                                                    threads which have returned no longer join
 *
 * Dynamic shared memory is a host array of the wrapper file; before every block the launcher
 * fills the requested bytes with a NaN pattern and the rest with a guard pattern, and checks
 * the guard afterwards.  Every entry point returns refshim::take_error(): 0, or a bit set of
 * REFSHIM_ERR_*.
 */
#ifndef MFSR_REFSHIM_LAUNCH_H
#define MFSR_REFSHIM_LAUNCH_H

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "cuda_runtime.h"

enum {
    REFSHIM_ERR_BARRIER_IN_LOOP = 1,   /* __syncthreads() under run(): the kernel needs run_threads() */
    REFSHIM_ERR_SHARED_TOO_LARGE = 2,  /* more dynamic shared memory requested than the wrapper file holds */
    REFSHIM_ERR_SHARED_GUARD = 4,      /* a block wrote past the shared memory it asked for */
    REFSHIM_ERR_BAD_BLOCK = 8          /* empty block, or more threads than run_threads() allows */
};

#define REFSHIM_EXPORT extern "C" __attribute__((visibility("default")))

namespace refshim {

constexpr size_t kSharedBytes = 48 * 1024;   /* per block, the CUDA default limit */
constexpr size_t kGuardBytes = 256;
constexpr unsigned kMaxHostThreads = 256;

struct shared_mem {
    void* base = nullptr;   /* kSharedBytes + kGuardBytes of host memory, or null */
    size_t bytes = 0;       /* what the launch asks for */
};

inline std::atomic<int> g_error{0};
inline void raise(int e) { g_error.fetch_or(e); }
inline int take_error() { return g_error.exchange(0); }

/* the barrier __syncthreads() reaches: null under run() */
struct block_barrier;
inline thread_local block_barrier* t_barrier = nullptr;

struct block_barrier {
    std::mutex m;
    std::condition_variable cv;
    unsigned live = 0, waiting = 0, generation = 0;
    void reset(unsigned n) { live = n; waiting = 0; }
    void release_locked() { waiting = 0; generation++; cv.notify_all(); }
    void wait()
    {
        std::unique_lock<std::mutex> lock(m);
        unsigned g = generation;
        if (++waiting == live) release_locked();
        else cv.wait(lock, [&] { return generation != g; });
    }
    void leave()   /* the thread has returned from the kernel */
    {
        std::unique_lock<std::mutex> lock(m);
        live--;
        if (live > 0 && waiting == live) release_locked();
    }
};

inline void barrier()
{
    if (t_barrier) t_barrier->wait();
    else raise(REFSHIM_ERR_BARRIER_IN_LOOP);
}

inline bool prepare_shared(const shared_mem& s)
{
    if (!s.base) return true;
    if (s.bytes > kSharedBytes) { raise(REFSHIM_ERR_SHARED_TOO_LARGE); return false; }
    memset(s.base, 0xFF, s.bytes);                                            /* uninitialised reads come back NaN */
    memset(static_cast<char*>(s.base) + s.bytes, 0x5A, kSharedBytes + kGuardBytes - s.bytes);
    return true;
}

inline void check_shared(const shared_mem& s)
{
    if (!s.base) return;
    const unsigned char* p = static_cast<const unsigned char*>(s.base);
    for (size_t i = s.bytes; i < kSharedBytes + kGuardBytes; i++)
        if (p[i] != 0x5A) { raise(REFSHIM_ERR_SHARED_GUARD); return; }
}

inline bool set_launch(dim3 grid, dim3 block)
{
    if (block.x * block.y * block.z == 0 || grid.x * grid.y * grid.z == 0) { raise(REFSHIM_ERR_BAD_BLOCK); return false; }
    gridDim = grid;
    blockDim = block;
    return true;
}

template <class Body>
int run(dim3 grid, dim3 block, shared_mem shared, Body&& body)
{
    if (!set_launch(grid, block)) return take_error();
    t_barrier = nullptr;
    for (unsigned bz = 0; bz < grid.z; bz++)
        for (unsigned by = 0; by < grid.y; by++)
            for (unsigned bx = 0; bx < grid.x; bx++) {
                blockIdx = {bx, by, bz};
                if (!prepare_shared(shared)) return take_error();
                for (unsigned tz = 0; tz < block.z; tz++)
                    for (unsigned ty = 0; ty < block.y; ty++)
                        for (unsigned tx = 0; tx < block.x; tx++) {
                            threadIdx = {tx, ty, tz};
                            body();
                        }
                check_shared(shared);
            }
    return take_error();
}

template <class Body>
int run(dim3 grid, dim3 block, Body&& body) { return run(grid, block, shared_mem(), body); }

/* Each of the block's host threads plays its (tx,ty,tz) for every block of the grid in turn;
 * `all` separates the blocks, `inner` is the kernel's own barrier. */
template <class Body>
int run_threads(dim3 grid, dim3 block, shared_mem shared, Body&& body)
{
    const unsigned n = block.x * block.y * block.z;
    if (n == 0 || n > kMaxHostThreads || grid.x * grid.y * grid.z == 0) { raise(REFSHIM_ERR_BAD_BLOCK); return take_error(); }
    if (shared.base && shared.bytes > kSharedBytes) { raise(REFSHIM_ERR_SHARED_TOO_LARGE); return take_error(); }
    block_barrier all, inner;
    all.reset(n);
    auto worker = [&](unsigned tx, unsigned ty, unsigned tz) {
        const bool first = (tx | ty | tz) == 0;
        gridDim = grid;
        blockDim = block;
        threadIdx = {tx, ty, tz};
        t_barrier = &inner;
        for (unsigned bz = 0; bz < grid.z; bz++)
            for (unsigned by = 0; by < grid.y; by++)
                for (unsigned bx = 0; bx < grid.x; bx++) {
                    blockIdx = {bx, by, bz};
                    if (first) { inner.reset(n); prepare_shared(shared); }
                    all.wait();
                    body();
                    inner.leave();
                    all.wait();
                    if (first) check_shared(shared);
                }
        t_barrier = nullptr;
    };
    std::vector<std::thread> pool;
    pool.reserve(n);
    for (unsigned tz = 0; tz < block.z; tz++)
        for (unsigned ty = 0; ty < block.y; ty++)
            for (unsigned tx = 0; tx < block.x; tx++) pool.emplace_back(worker, tx, ty, tz);
    for (auto& t : pool) t.join();
    return take_error();
}

inline unsigned cdiv(int n, int d) { return n <= 0 ? 1u : (unsigned)((n + d - 1) / d); }

/* texture descriptors of a wrapper: `cfg` packs, four bits per texture in argument order,
 * bit 0 = address mode, bit 1 = filter variant */
inline refshim_tex make_tex(const void* ptr, int pitch, int w, int h, int cfg, int index)
{
    int bits = (cfg >> (4 * index)) & 15;
    refshim_tex t = {ptr, pitch, w, h, bits & 1, (bits >> 1) & 1};
    return t;
}
inline cudaTextureObject_t handle(const refshim_tex& t) { return static_cast<cudaTextureObject_t>(reinterpret_cast<uintptr_t>(&t)); }

} // namespace refshim

#endif
