// The launch policy (miniworld_amd/csrc/mw_policy.h) compiled for the host: tests/test_launch_policy_cpu.py asks it for the decisions
// of a table of cases and compares them with the answers recorded from the runtime before the policy was split out of it.
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace mwpolicy;

// what: the question; in / out: its integers.  Returns the number of answers, -1 for an unknown question.
extern "C" int mwpol(int what, const long long *in, long long *out)
{
    const auto I = [&](int k) { return (int)in[k]; };
    const auto B = [&](int k) { return in[k] != 0; };
    switch (what) {
    case 0: {   // msaa, W, H, meshes, order, MW_K2Q, MW_GENERIC_RASTER, layout, debug flags, depth, the quad kernel's LDS bytes
        const bool ok = k2q_ok(I(0), I(1), I(2), I(10));
        const RasterPath p = raster_path({I(0), I(1), I(2), B(3), B(4), B(5), B(6), ok, I(7), I(8)}, B(9));
        const long long r[] = {p.path, p.mesh, p.quad4, p.big, p.general, p.ragged, p.depth, ok};
        for (int k = 0; k < 8; ++k) out[k] = r[k];
        return 8;
    }
    case 1: {   // max_polys, max_ents, max_visible, task, num_envs, n_tiles
        const int E = I(1) > 1 ? I(1) : 1;
        out[0] = geom_lanes(I(0), E, has_visiting_order(I(2))); out[1] = k1_dense_lanes(I(0), E, I(2), I(3)); out[2] = pick_waves_per_env(I(5), I(4));
        return 3;
    }
    case 2: {   // call kind, view_flags, reuse on, held match, meshes, debug flags, layout, task, cache allocated, path
        const FramePolicy p = frame_policy({(CallKind)I(0), I(1), B(2), B(3), B(4), I(5), I(6), I(7), B(8), I(9)});
        out[0] = p.reuse; out[1] = p.source; out[2] = p.cache; out[3] = p.hold;
        return 4;
    }
    case 3: out[0] = stack_phase(in[1], I(0)); return 1;        // depth, pushes
    case 4: {   // obs, ring, final_obs, final_stack, frame_bytes
        const StackLaunch s = stack_launch((uintptr_t)(in[0] | in[1] | in[2] | in[3]), (size_t)in[4]);
        out[0] = s.wide; out[1] = s.chunks;
        return 2;
    }
    case 5: {   // count, total_rows, chunks_per_item
        const SnapshotGrid g = snapshot_grid(I(0), I(1), I(2));
        out[0] = g.item_chunks; out[1] = g.blocks; out[2] = g.blocks < 0 || grid_too_large((unsigned long long)g.blocks); out[3] = (unsigned)(g.blocks > 1 ? g.blocks : 1);
        return 4;
    }
    case 6: {   // the addresses or'ed, frame_bytes, depth_bytes, stack_depth, count
        const SnapfGrid g = snapf_grid((uintptr_t)in[0], (uint64_t)in[1], (uint64_t)in[2], I(3), I(4));
        out[0] = g.wide; out[1] = (long long)g.frame_chunks; out[2] = (long long)g.depth_chunks; out[3] = (long long)g.per_item; out[4] = (long long)g.blocks;
        return 5;
    }
    case 7: {   // part, tile list, big, max_vis, n_tiles, waves per env, N, the mesh tiles' wavefronts
        const TileLaunch t = tile_launch(I(0), B(1), B(2), I(3), I(4), I(5), I(6), I(7));
        out[0] = t.part; out[1] = t.waves_per_env; out[2] = t.tiles_per_wave; out[3] = t.grid; out[4] = (long long)t.lds;
        return 5;
    }
    case 8: {   // generator, autoreset
        const ResetMode m = reset_mode(I(0), I(1));
        out[0] = m.installs; out[1] = m.same; out[2] = m.next;
        return 3;
    }
    case 9:     // MW_DEBUG_FLAGS, layout, part, stamp, reuse, W, H
        out[0] = raster_flags(I(0) & MW_DEBUG_BITS, I(1), I(2), (uint32_t)in[3], B(4)); out[1] = (long long)obs_row_bytes(I(5), I(6), I(1));
        return 2;
    case 10:    // W, H
        out[0] = tile_kernels_exact(I(0), I(1)); out[1] = frame_on_grid(I(0), I(1)); out[2] = tile_path_ok(I(0), I(1)); out[3] = frame_size_ok(I(0), I(1));
        return 4;
    }
    return -1;
}
