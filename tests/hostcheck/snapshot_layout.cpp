// The snapshot record layout (miniworld_amd/csrc/mw_snapshot.h) compiled for the host: tests/test_snapshot_cpu.py reads the sections
// of a buffer from here and checks that they are disjoint, aligned and add up to what mw_snapshot_bytes returns.
#include "../../miniworld_amd/csrc/mw_snapshot.h"

namespace {
MwSnapConfig config_of(const int32_t *c) { return {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]}; }
}

extern "C" {

// cfg: E, max_polys, max_segs, shared_geom, task, generator, rng_mode, spares, health.  Fills, per section of a buffer of `capacity`
// records (the blobs the configuration has, then its components in MW_SC_* order): the offset, the bytes, the alignment its copies
// need (16: moved in 16-byte units; else the element size) and the component id (-1 - blob for a blob).  Returns the sections.
int mwsnap_sections(const int32_t *cfg, long long capacity, unsigned long long *off, unsigned long long *bytes, int *align, int *id, int max)
{
    const MwSnapLayout L = mw_snap_layout(config_of(cfg));
    int n = 0;
    for (int b = 0; b < MW_SB_COUNT; ++b)
        if (L.blob_bytes[b] && n < max) {
            off[n] = mw_snap_offset(L.blob_unit[b], capacity); bytes[n] = L.blob_bytes[b] * (unsigned long long)capacity; align[n] = 16; id[n] = -1 - b;
            ++n;
        }
    for (int c = 0; c < MW_SC_COUNT; ++c)
        if (L.comp_rows[c] && n < max) {
            off[n] = mw_snap_offset(L.comp_unit[c], capacity);
            bytes[n] = (unsigned long long)L.comp_rows[c] * L.comp_elem[c] * (unsigned long long)capacity; align[n] = L.comp_elem[c]; id[n] = c;
            ++n;
        }
    return n;
}

long long mwsnap_bytes(const int32_t *cfg, long long capacity) { return mw_snap_bytes(mw_snap_layout(config_of(cfg)), capacity); }
int mwsnap_total_rows(const int32_t *cfg) { return mw_snap_layout(config_of(cfg)).total_rows; }
int mwsnap_header_bytes(void) { return MW_SNAP_HEADER_BYTES; }
void mwsnap_key(const int32_t *cfg, int capacity, unsigned *out)
{
    const MwSnapKey k = mw_snap_key(config_of(cfg), capacity);
    for (int i = 0; i < MW_SNAP_KEY_WORDS; ++i) out[i] = k.w[i];
}

}
