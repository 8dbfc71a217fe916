// Frame records (mw_snapshot_save_frames / mw_snapshot_load_frames): an env's rows of the caller's observation and depth buffers and its
// frame stack out into a caller's buffer and back — what lets a fork carry the frames it already has instead of drawing them again.
// A pure copy: no arithmetic, nothing but loads, stores and index tests.  The layout of the buffer: mw_snapframes.h.
// The forms with chosen records (_at) and with a device mask over all envs (_where) are the same two kernels: the items are named by
// d_envs, d_recs and mask (MW_SNAP_ITEMS, mw_kernels.h).
//
// One launch per call, a 1-D grid: workgroup (item, chunk of the record), the chunks of an item being those of its obs row, of its
// depth row and of its K window frames.  What happens to an item — index valid, key equal, which part a chunk belongs to — is uniform
// per workgroup.  There is no barrier and no LDS.  A unit is 16 bytes when the frame sizes and every base are multiples of 16 (`wide`,
// the switch of mw_stack.hip), else a byte.
//
// The stack travels in WINDOW order: frame k of a record is the env's k-th oldest frame, read from ring slot first + k.  A load writes
// it to slot first + k of the engine's CURRENT window and to the mirror slot K away where that lies inside 0 .. 2K - 2 — the two slots
// a push writes (mw_stack.hip) —, which covers all 2K - 1 slots: the row is the one the env would have had it pushed those K frames
// itself, so this window and every later one are right and the ring position does not move.  The lane that read a unit stores it to
// both slots, so the chunks of an env cannot race.
#include <hip/hip_runtime.h>

#include "mw_kernels.h"

namespace {

template <typename T> __device__ __forceinline__ T no_unit();
template <> __device__ __forceinline__ uint4 no_unit<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }
template <> __device__ __forceinline__ uint8_t no_unit<uint8_t>() { return 0; }

// one chunk of `units` units from src to dst and, where there is one, to dst2
template <typename T>
__device__ __forceinline__ void copy_chunk(uint8_t *dst_bytes, uint8_t *dst2_bytes, const uint8_t *src_bytes, size_t units, int chunk)
{
    T *dst = reinterpret_cast<T *>(dst_bytes), *dst2 = reinterpret_cast<T *>(dst2_bytes);
    const T *src = reinterpret_cast<const T *>(src_bytes);
    const size_t first = (size_t)chunk * (MW_SNAPF_THREADS * MW_SNAPF_UNROLL) + threadIdx.x;
    // the four loads first, then the stores (named values: an array indexed in a loop was given a place in LDS by the compiler,
    // mw_snapshot.hip)
    static_assert(MW_SNAPF_UNROLL == 4, "the copy is written out for four units per lane");
    const size_t u0 = first, u1 = first + MW_SNAPF_THREADS, u2 = first + 2 * MW_SNAPF_THREADS, u3 = first + 3 * MW_SNAPF_THREADS;
    T v0 = no_unit<T>(), v1 = v0, v2 = v0, v3 = v0;
    if (u0 < units) v0 = src[u0];
    if (u1 < units) v1 = src[u1];
    if (u2 < units) v2 = src[u2];
    if (u3 < units) v3 = src[u3];
    if (u0 < units) dst[u0] = v0;
    if (u1 < units) dst[u1] = v1;
    if (u2 < units) dst[u2] = v2;
    if (u3 < units) dst[u3] = v3;
    if (dst2) {
        if (u0 < units) dst2[u0] = v0;
        if (u1 < units) dst2[u1] = v1;
        if (u2 < units) dst2[u2] = v2;
        if (u3 < units) dst2[u3] = v3;
    }
}

// LOAD: the engine side (obs, depth, ring, stack_flags) is written from `frames`; else the other way round
template <bool LOAD, typename T>
__device__ __forceinline__ void frames_block(const MwSnapfArgs &a, const int32_t *__restrict__ d_envs, const int32_t *__restrict__ d_recs,
                                             uint8_t *obs, uint8_t *depth, uint8_t *ring, uint8_t *stack_flags, uint8_t *frames,
                                             uint32_t *__restrict__ status, const uint8_t *__restrict__ mask)
{
    const int k = (int)(blockIdx.x / (unsigned)a.chunks_per_item), c = (int)(blockIdx.x % (unsigned)a.chunks_per_item);
    if (k >= a.count) return;
    if (mask && !mask[k]) return;
    const int env = d_envs ? d_envs[k] : k;
    const int rec = d_recs ? d_recs[k] : k;
    if ((unsigned)env >= (unsigned)a.N || (unsigned)rec >= (unsigned)a.n_recs) {
        if (c == 0 && threadIdx.x == 0) atomicOr(status, MW_ST_SNAPSHOT_BAD);
        return;
    }
    const size_t fb = (size_t)a.frame_bytes, db = (size_t)a.depth_bytes, e = (size_t)env, r = (size_t)rec;
    uint8_t *in_engine, *in_engine2 = nullptr, *in_record;
    size_t bytes;
    int chunk;
    if (c < a.frame_chunks) {
        chunk = c; bytes = fb;
        in_engine = obs + e * fb;
        in_record = frames + a.off[MW_SF_OBS] + r * fb;
        // the env's stack flag byte goes with its first chunk (a load: into the current half, like mw_snapshot_load's mark)
        if (a.stack_depth && c == 0 && threadIdx.x == 0) {
            uint8_t *flag_rec = frames + a.off[MW_SF_STACK_FLAG] + r;
            if (LOAD) stack_flags[e] = *flag_rec; else *flag_rec = stack_flags[e];
        }
    } else if (c < a.frame_chunks + a.depth_chunks) {
        chunk = c - a.frame_chunks; bytes = db;
        in_engine = depth + e * db;
        in_record = frames + a.off[MW_SF_DEPTH] + r * db;
    } else {
        const int s = c - a.frame_chunks - a.depth_chunks, K = a.stack_depth;
        const int w = s / a.frame_chunks, slot = a.first_slot + w;      // window frame w, 0 .. K - 1; slot 0 .. 2K - 2
        chunk = s % a.frame_chunks; bytes = fb;
        uint8_t *ring_env = ring + e * (size_t)(2 * K - 1) * fb;
        in_engine = ring_env + (size_t)slot * fb;
        if (LOAD && slot >= K) in_engine2 = ring_env + (size_t)(slot - K) * fb;
        else if (LOAD && slot + K <= 2 * K - 2) in_engine2 = ring_env + (size_t)(slot + K) * fb;
        in_record = frames + a.off[MW_SF_STACK] + (r * (size_t)K + (size_t)w) * fb;
    }
    if (LOAD) copy_chunk<T>(in_engine, in_engine2, in_record, bytes / sizeof(T), chunk);
    else copy_chunk<T>(in_record, nullptr, in_engine, bytes / sizeof(T), chunk);
}

// the header: the key, then zeros, by one lane of the first workgroup (every save writes it, an empty one too)
__device__ __forceinline__ void write_header(const MwSnapfKey &key, uint8_t *frames)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint32_t *head = reinterpret_cast<uint32_t *>(frames);
#pragma unroll
        for (int i = 0; i < MW_SNAPF_KEY_WORDS; ++i) head[i] = key.w[i];
#pragma unroll
        for (int i = MW_SNAPF_KEY_WORDS; i < MW_SNAPF_HEADER_BYTES / 4; ++i) head[i] = 0u;
    }
}

// a buffer of another layout (or no frame records at all): nothing of it is read beyond its first words, nothing is written
__device__ __forceinline__ bool key_matches(const MwSnapfKey &key, const uint8_t *frames, uint32_t *__restrict__ status)
{
    const uint32_t *head = reinterpret_cast<const uint32_t *>(frames);
    bool same = true;
#pragma unroll
    for (int i = 0; i < MW_SNAPF_KEY_WORDS; ++i) same = same && head[i] == key.w[i];
    if (!same && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, MW_ST_SNAPSHOT_BAD);
    return same;
}

}  // namespace

extern "C" __global__ __launch_bounds__(MW_SNAPF_THREADS) void mw_snapshot_save_frames_kernel(MW_SNAPF_ARGS, const uint8_t *__restrict__ obs,
                                                                                             const uint8_t *__restrict__ depth, const uint8_t *__restrict__ ring,
                                                                                             const uint8_t *__restrict__ stack_flags, uint8_t *__restrict__ frames,
                                                                                             MW_SNAP_ITEMS)
{
    write_header(a.key, frames);
    // (the engine side is only read: frames_block<false> never writes through these pointers)
    uint8_t *o = const_cast<uint8_t *>(obs), *d = const_cast<uint8_t *>(depth), *g = const_cast<uint8_t *>(ring), *f = const_cast<uint8_t *>(stack_flags);
    if (a.wide) frames_block<false, uint4>(a, d_envs, d_recs, o, d, g, f, frames, status, mask);
    else frames_block<false, uint8_t>(a, d_envs, d_recs, o, d, g, f, frames, status, mask);
}

extern "C" __global__ __launch_bounds__(MW_SNAPF_THREADS) void mw_snapshot_load_frames_kernel(MW_SNAPF_ARGS, const uint8_t *__restrict__ frames,
                                                                                             uint8_t *__restrict__ obs, uint8_t *__restrict__ depth,
                                                                                             uint8_t *__restrict__ ring, uint8_t *__restrict__ stack_flags,
                                                                                             MW_SNAP_ITEMS)
{
    if (!key_matches(a.key, frames, status)) return;
    uint8_t *f = const_cast<uint8_t *>(frames);
    if (a.wide) frames_block<true, uint4>(a, d_envs, d_recs, obs, depth, ring, stack_flags, f, status, mask);
    else frames_block<true, uint8_t>(a, d_envs, d_recs, obs, depth, ring, stack_flags, f, status, mask);
}
