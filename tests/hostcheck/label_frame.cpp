// The host path of miniworld_amd/csrc/mw_label.h, as a program of its own (tests/test_label_cpu.py builds it with the address and
// undefined-behaviour sanitizers): one env's polygons, entity slots and meshes from a file, then a list of poses and cameras, each one
// mwlabel::frame_env<HostOps> with (lane, stride) = (0, 1) into the same buffers — the kernel's phases, pruning rectangle and bands
// included (a step under a zero mask byte is skipped, as the kernel skips the env).
//
// The file (hostcheck.h: the tokens, the world block; floats as the hexadecimal bits of their float32):
//   W H msaa  near far flags  band_rows chunk          (band_rows, chunk 0: mwpolicy::label_launch's)
//   npolys, then per polygon: nv (with its MW_POLY_* flags), 12 words v, 4 words xf
//   the world: SLOTS in their WIDE form alone
//   nmesh, then per mesh: ntris and 9 * ntris words
//   garbage                    (the byte every output holds before the first step)
//   nsteps, then per step: x y z dir  cam_height cam_fwd_disp cam_pitch cam_fov_y  mask
// The answer, per step, five lines: H * W classes, H * W codes, the H * W depths as hexadecimal bits, E pixel counts, 4 * E box words.
// `label_frame --policy N W H max_polys max_ents` prints mwpolicy::label_launch instead: "grid threads lds band_rows chunk fits".
#define HOSTCHECK_PROGRAM "label_frame"
#include "hostcheck.h"

#include "../../miniworld_amd/csrc/mw_label.h"
#include "../../miniworld_amd/csrc/mw_policy.h"

using namespace hostcheck;

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "--policy")) {
        const mwpolicy::LabelLaunch l = mwpolicy::label_launch(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
        printf("%llu %d %zu %d %d %d\n", l.grid, l.threads, l.lds, l.band_rows, l.chunk, l.fits ? 1 : 0);
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: label_frame SCENE | label_frame --policy N W H max_polys max_ents\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    const int W = ri(f), H = ri(f), msaa = ri(f);
    mw_label_params p{};
    p.near = rd(f); p.far = rd(f); p.flags = ri(f);
    int band_rows = ri(f), chunk = ri(f);
    const int npolys = ri(f);
    if (W < 1 || H < 1 || (msaa != 1 && msaa != 4 && msaa != 8) || !(p.near >= 0.0) || !(p.near < p.far) || (p.flags & ~(MW_LABEL_MESH_BOUNDS | MW_LABEL_UNPRUNED)) ||
        npolys < 0 || npolys > MW_LABEL_MAX_POLYS)
        return refused();
    std::vector<mw_poly> polys((size_t)npolys);
    for (mw_poly &q : polys) {
        memset(&q, 0, sizeof q);
        q.nv = ri(f);
        for (int i = 0; i < 4; ++i) for (int k = 0; k < 3; ++k) q.v[i][k] = rbits(f);
        for (int k = 0; k < 4; ++k) q.xf[k] = rbits(f);
    }
    World world;
    if (!world.read(f, SLOTS | WIDE, MW_LABEL_MAX_ENTS)) return refused();
    const int E = world.E;
    const int nmesh = ri(f);
    std::vector<MwMeshDesc> descs((size_t)(nmesh > 0 ? nmesh : 0));
    std::vector<float> pool;
    for (int m = 0; m < nmesh; ++m) {
        const int ntris = ri(f);
        memset(&descs[m], 0, sizeof descs[m]);
        descs[m].ntris = (uint32_t)ntris;
        descs[m].first = (uint32_t)(pool.size() / MW_MESH_POS_STRIDE);
        for (int t = 0; t < ntris; ++t) {
            for (int k = 0; k < 9; ++k) pool.push_back(rbits(f));
            pool.push_back(0.0f);
        }
    }
    const int garbage = ri(f);
    const mwpolicy::LabelLaunch l = mwpolicy::label_launch(1, W, H, npolys, E);
    if (!l.fits) { fprintf(stderr, "label_frame: a frame or scene the engine refuses\n"); return 2; }
    if (band_rows < 1) band_rows = l.band_rows;
    if (chunk < 1) chunk = l.chunk;
    int32_t np = npolys;
    double ay = 0.0, cam[4] = {0.0, 0.0, 0.0, 0.0};
    MwLabelArgs a{};
    a.r = world.ray();
    a.ay = &ay; a.cam = cam; a.edir = world.edir.data(); a.emesh = world.emesh.data(); a.polys = polys.data(); a.npolys = &np;
    a.mesh = nmesh > 0 ? descs.data() : nullptr; a.mesh_pos = nmesh > 0 ? pool.data() : nullptr;
    a.max_polys = npolys; a.n_mesh = nmesh; a.W = W; a.H = H; a.msaa = msaa;
    const size_t pixels = (size_t)W * H;
    std::vector<uint8_t> cls(pixels, (uint8_t)garbage);
    std::vector<int32_t> code(pixels), pix((size_t)E), box((size_t)E * 4);
    std::vector<float> depth(pixels);
    memset(code.data(), garbage, code.size() * 4);
    memset(depth.data(), garbage, depth.size() * 4);
    if (E) { memset(pix.data(), garbage, pix.size() * 4); memset(box.data(), garbage, box.size() * 4); }
    const size_t bytes = mwlabel::plan_bytes(band_rows * W, chunk, E);
    void *lds = aligned_alloc(16, bytes);
    if (!lds) return 2;
    const mwlabel::Out out{cls.data(), code.data(), depth.data(), pix.data(), box.data()};
    const int nsteps = ri(f);
    for (int t = 0; t < nsteps; ++t) {
        world.ax = rd(f); ay = rd(f); world.az = rd(f); world.adir = rd(f);
        for (double &v : cam) v = rd(f);
        if (ri(f) != 0) mwlabel::frame_env<mwlabel::HostOps>(a, p, 0, lds, band_rows, chunk, !(p.flags & MW_LABEL_UNPRUNED), out, 0, 1);
        for (size_t k = 0; k < pixels; ++k) printf("%u%s", (unsigned)cls[k], k + 1 == pixels ? "" : " ");
        printf("\n");
        for (size_t k = 0; k < pixels; ++k) printf("%d%s", (int)code[k], k + 1 == pixels ? "" : " ");
        printf("\n");
        for (size_t k = 0; k < pixels; ++k) { uint32_t u; memcpy(&u, &depth[k], 4); printf("%x%s", (unsigned)u, k + 1 == pixels ? "" : " "); }
        printf("\n");
        for (int s = 0; s < E; ++s) printf("%d%s", (int)pix[s], s + 1 == E ? "" : " ");
        printf("\n");
        for (int s = 0; s < 4 * E; ++s) printf("%d%s", (int)box[s], s + 1 == 4 * E ? "" : " ");
        printf("\n");
    }
    free(lds);
    fclose(f);
    return 0;
}
