// Snapshot records (mw_snapshot_save / mw_snapshot_load): the complete state of an env out of the engine's arrays into a caller's
// buffer and back — the hot path of a fork loop (tree search, particle resampling: save the batch, load it back through an index).
// A pure copy: no arithmetic, nothing but loads, stores and index tests.  The layout of the buffer: mw_snapshot.h.
// The forms with chosen records (mw_snapshot_save_at) and with a device mask over all envs (mw_snapshot_load_where) are the same two
// kernels: which of d_envs, d_recs and mask is null names the items (MW_SNAP_ITEMS, mw_kernels.h) — a level bank filled in chunks, and
// the envs a step finished — known on the device alone — restarted from it.
//
// One launch per call, a 1-D grid of two kinds of workgroups, told apart by blockIdx alone:
//   component blocks  (row r of the state, 256 consecutive items): the engine's state is component-major over the envs and the
//       records are component-major over the records, so lane t moves ONE element of item chunk * 256 + t — the side that is
//       addressed by the item itself (the records of a save, both sides of a whole-batch call) is a contiguous run per
//       wavefront, the side addressed through d_envs / d_recs a gather or scatter of whole elements.  Which component a row
//       belongs to is read from the engine's table (row -> component, uniform per workgroup: two scalar loads).
//   blob blocks  (item, geometry set, chunk), per-env geometry sets only: an env's polygons and segments are contiguous, so a
//       workgroup moves a chunk of MW_SNAP_THREADS * MW_SNAP_UNROLL 16-byte units of them — up to the set's OWN polygon / segment
//       count, read from the source side and clamped to the capacity: nothing ever reads a set past its count (the geometry
//       kernel, the collision tests and take_spare all stop there; mw_get_geometry returns the count with the array).
// There is no barrier and no LDS.  What a blob block decides per item (index valid, chunk inside the count) is uniform per workgroup;
// a component block's lanes each test their own item — consecutive lanes, consecutive items — and an invalid one just sits out.
// The header's key (a load) is compared by every workgroup before anything else: all of them leave on a mismatch.
//
// Between launches refill_mask is 0 (spare ready) or 1 (consumed, refill pending) only: the transient states 2 and 3 exist inside a
// step kernel or a refill kernel, and both calls are ordered behind those (mw_engine_snapshot.hip: snapshot_order).  The word is copied as it is.
#include <hip/hip_runtime.h>

#include "mw_kernels.h"

namespace {

struct Item { int env, rec; bool ok; };

// item k of the call (MW_SNAP_ITEMS; the caller has seen that it is present): the env and the record, each tested against its limit
__device__ __forceinline__ Item item_of(int k, int N, int n_recs, const int32_t *__restrict__ d_envs, const int32_t *__restrict__ d_recs)
{
    Item it;
    it.env = d_envs ? d_envs[k] : k;
    it.rec = d_recs ? d_recs[k] : k;
    it.ok = (unsigned)it.env < (unsigned)N && (unsigned)it.rec < (unsigned)n_recs;
    return it;
}

template <typename T>
__device__ __forceinline__ void move(void *dst, const void *src) { *static_cast<T *>(dst) = *static_cast<const T *>(src); }

// (fc_epoch: null, or the frame-cache epoch a written env advances)
template <bool LOAD>
__device__ __forceinline__ void snapshot_block(const MwSnapTable *__restrict__ tab, int N, int capacity, int count, int item_chunks,
                                               const int32_t *__restrict__ d_envs, const int32_t *__restrict__ d_recs, int n_recs,
                                               uint32_t *__restrict__ status, uint8_t *snap, uint8_t *__restrict__ frame_clean,
                                               int32_t *__restrict__ occ_valid, uint8_t *__restrict__ stack_flags,
                                               const uint8_t *__restrict__ mask, uint32_t *__restrict__ fc_epoch)
{
    const int tid = (int)threadIdx.x;
    const int total_rows = tab->total_rows;
    const long long comp_blocks = (long long)item_chunks * total_rows;
    const size_t cap = (size_t)capacity;
    if ((long long)blockIdx.x < comp_blocks) {
        // ---- a row of a component, 256 items
        const int row = (int)(blockIdx.x / (unsigned)item_chunks), chunk = (int)(blockIdx.x % (unsigned)item_chunks);
        const MwSnapRow comp = tab->comp[tab->row_comp[row]];
        const int k = chunk * MW_SNAP_THREADS + tid;
        if (k >= count) return;
        if (mask && !mask[k]) return;
        const Item it = item_of(k, N, n_recs, d_envs, d_recs);
        if (!it.ok) {
            if (row == 0) atomicOr(status, MW_ST_SNAPSHOT_BAD);
            return;
        }
        const size_t r = (size_t)(row - comp.row0), elem = (size_t)comp.elem;
        uint8_t *in_engine = static_cast<uint8_t *>(comp.eng) + (r * (size_t)N + (size_t)it.env) * elem;
        uint8_t *in_record = snap + MW_SNAP_HEADER_BYTES + cap * comp.unit + (r * cap + (size_t)it.rec) * elem;
        void *dst = LOAD ? in_engine : in_record;
        const void *src = LOAD ? in_record : in_engine;
        if (comp.elem == 8) move<uint64_t>(dst, src);
        else if (comp.elem == 4) move<uint32_t>(dst, src);
        else move<uint8_t>(dst, src);
        if (LOAD && row == 0) {
            // what else a load owes every env it writes: its frame is no longer the one in d_obs, the culling data of its geometry
            // set belongs to the polygons that were there, and its frame stack starts over like after mw_reset (a pending
            // next-step reset of the record keeps its mark: the push of the call that installs the world rebuilds again)
            frame_clean[it.env] = 0;
            if (occ_valid) occ_valid[it.env] = 0;
            if (stack_flags) {
                const uint8_t pending = snap[MW_SNAP_HEADER_BYTES + cap * tab->reset_pending_unit + (size_t)it.rec];
                stack_flags[it.env] = (uint8_t)(MW_STACK_FRESH | (pending ? MW_STACK_PENDING : 0));
            }
            // ... and the masked form, which leaves the host's cache-wide invalidation out: no cached frame of the env matches again
            // (the epoch is part of the key and of no record, MwArgs::fc_epoch)
            if (fc_epoch) fc_epoch[it.env] += 1u;
        }
        return;
    }
    // ---- a chunk of one geometry set of one item
    const int n_geo = tab->n_geo;
    if (n_geo == 0) return;
    const int poly_chunks = tab->poly_chunks, per_set = poly_chunks + tab->seg_chunks, per_item = n_geo * per_set;
    const long long g = (long long)blockIdx.x - comp_blocks;
    const int k = (int)(g / per_item), within = (int)(g % per_item);
    if (k >= count) return;
    if (mask && !mask[k]) return;
    const Item it = item_of(k, N, n_recs, d_envs, d_recs);
    if (!it.ok) return;         // (the status bit: the item's component block of row 0)
    const int set = within / per_set, part = within % per_set;
    const bool polys = part < poly_chunks;
    const int chunk = polys ? part : part - poly_chunks;
    // the set's own count, from the side that is read; never past the capacity
    const int32_t *eng_n = polys ? tab->eng_npolys[set] : tab->eng_nsegs[set];
    const uint64_t n_unit = polys ? tab->npolys_unit[set] : tab->nsegs_unit[set];
    const int32_t *rec_n = reinterpret_cast<const int32_t *>(snap + MW_SNAP_HEADER_BYTES + cap * n_unit);
    const int limit = polys ? tab->max_polys : tab->max_segs;
    int n = LOAD ? rec_n[it.rec] : eng_n[it.env];
    n = n < 0 ? 0 : n > limit ? limit : n;
    const size_t units_each = polys ? MW_SNAP_POLY_BYTES / 16 : MW_SNAP_SEG_BYTES / 16;
    const size_t units = (size_t)n * units_each, blob_units = (size_t)limit * units_each;
    uint4 *in_engine = static_cast<uint4 *>(polys ? tab->eng_polys[set] : tab->eng_segs[set]) + (size_t)it.env * blob_units;
    uint4 *in_record = reinterpret_cast<uint4 *>(snap + MW_SNAP_HEADER_BYTES + cap * (polys ? tab->polys_unit[set] : tab->segs_unit[set])) + (size_t)it.rec * blob_units;
    uint4 *dst = LOAD ? in_engine : in_record;
    const uint4 *src = LOAD ? in_record : in_engine;
    const size_t first = (size_t)chunk * (MW_SNAP_THREADS * MW_SNAP_UNROLL) + (size_t)tid;
    // the four loads first, then the four stores (named values: an array indexed in a loop was given a place in LDS by the compiler)
    static_assert(MW_SNAP_UNROLL == 4, "the blob copy is written out for four units per lane");
    const size_t u0 = first, u1 = first + MW_SNAP_THREADS, u2 = first + 2 * MW_SNAP_THREADS, u3 = first + 3 * MW_SNAP_THREADS;
    uint4 v0 = make_uint4(0u, 0u, 0u, 0u), v1 = v0, v2 = v0, v3 = v0;
    if (u0 < units) v0 = src[u0];
    if (u1 < units) v1 = src[u1];
    if (u2 < units) v2 = src[u2];
    if (u3 < units) v3 = src[u3];
    if (u0 < units) dst[u0] = v0;
    if (u1 < units) dst[u1] = v1;
    if (u2 < units) dst[u2] = v2;
    if (u3 < units) dst[u3] = v3;
}

// the header: the key, then zeros, by one lane of the first workgroup (every save writes it, an empty one too)
__device__ __forceinline__ void write_header(const MwSnapKey &key, uint8_t *snap)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint32_t *head = reinterpret_cast<uint32_t *>(snap);
#pragma unroll
        for (int i = 0; i < MW_SNAP_HEADER_BYTES / 4; ++i) head[i] = i < MW_SNAP_KEY_WORDS ? key.w[i < MW_SNAP_KEY_WORDS ? i : 0] : 0u;
    }
}

// a buffer of another layout (or no snapshot at all): nothing of it is read beyond its first words, nothing is written
__device__ __forceinline__ bool key_matches(const MwSnapKey &key, const uint8_t *snap, uint32_t *__restrict__ status)
{
    const uint32_t *head = reinterpret_cast<const uint32_t *>(snap);
    bool same = true;
#pragma unroll
    for (int i = 0; i < MW_SNAP_KEY_WORDS; ++i) same = same && head[i] == key.w[i];
    if (!same && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, MW_ST_SNAPSHOT_BAD);
    return same;
}

}  // namespace

// (a save: every record of the buffer may be written, n_recs is the capacity)
extern "C" __global__ __launch_bounds__(MW_SNAP_THREADS) void mw_snapshot_save_kernel(MW_SNAP_ARGS, uint8_t *__restrict__ snap, MW_SNAP_ITEMS)
{
    write_header(key, snap);
    snapshot_block<false>(tab, N, capacity, count, item_chunks, d_envs, d_recs, capacity, status, snap, nullptr, nullptr, nullptr, mask, nullptr);
}

extern "C" __global__ __launch_bounds__(MW_SNAP_THREADS) void mw_snapshot_load_kernel(MW_SNAP_ARGS, const uint8_t *__restrict__ snap, int n_recs,
                                                                                     uint8_t *__restrict__ frame_clean, int32_t *__restrict__ occ_valid,
                                                                                     uint8_t *__restrict__ stack_flags, uint32_t *__restrict__ fc_epoch,
                                                                                     MW_SNAP_ITEMS)
{
    if (!key_matches(key, snap, status)) return;
    snapshot_block<true>(tab, N, capacity, count, item_chunks, d_envs, d_recs, n_recs, status, const_cast<uint8_t *>(snap), frame_clean, occ_valid,
                         stack_flags, mask, fc_epoch);
}
