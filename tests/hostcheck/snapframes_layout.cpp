// The frame record layout (miniworld_amd/csrc/mw_snapframes.h) compiled for the host: tests/test_snapshot_frames_cpu.py reads the
// sections of a buffer from here and checks that they are disjoint, aligned and add up to what mw_snapshot_frames_bytes returns.
#include "../../miniworld_amd/csrc/mw_snapframes.h"

namespace {
// cfg: W, H, obs layout, flags, stack depth, bytes of a frame
MwSnapfConfig config_of(const long long *c) { return {(int32_t)c[0], (int32_t)c[1], (int32_t)c[2], (int32_t)c[3], (int32_t)c[4], (uint64_t)c[5]}; }
}

extern "C" {

// Fills, per section a buffer of `capacity` records has (obs, depth, stack, stack flags): the offset, the bytes of the section (whole
// 16-byte units), the bytes of one record's part of it and the section id (MW_SF_*).  Returns the sections.
int mwsnapf_sections(const long long *cfg, long long capacity, unsigned long long *off, unsigned long long *bytes, unsigned long long *rec_bytes,
                     int *id, int max)
{
    const MwSnapfLayout L = mw_snapf_layout(config_of(cfg), capacity);
    int n = 0;
    for (int s = 0; s < MW_SF_COUNT; ++s)
        if (L.rec_bytes[s] && n < max) {
            off[n] = L.off[s]; bytes[n] = L.bytes[s]; rec_bytes[n] = L.rec_bytes[s]; id[n] = s;
            ++n;
        }
    return n;
}

long long mwsnapf_bytes(const long long *cfg, long long capacity) { return (long long)mw_snapf_layout(config_of(cfg), capacity).total; }
int mwsnapf_header_bytes(void) { return MW_SNAPF_HEADER_BYTES; }
void mwsnapf_key(const long long *cfg, int capacity, unsigned *out)
{
    const MwSnapfKey k = mw_snapf_key(config_of(cfg), capacity);
    for (int i = 0; i < MW_SNAPF_KEY_WORDS; ++i) out[i] = k.w[i];
}

}
