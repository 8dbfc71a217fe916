// Device functions shared by the step kernels (mw_setup.hip: one wavefront per env, any scene; mw_setup_dense.hip:
// several envs per wavefront, small scenes) and the geometry kernel: the f64 dynamics of MiniWorldEnv.step
// (miniworld.py:606-730, 937-963; math.py:30-62), and the step itself (step_env), which both step kernels run.
#pragma once
#include "mw_device.h"
#include "mw_math.h"
#include "mw_rng.h"
#include "mw_gen.h"

namespace {

constexpr double kPi = 3.14159265358979323846;

__device__ inline uint64_t ballot(bool p) { return __ballot(p); }

// wave-uniform values computed on the VALU are moved to SGPRs so they do not occupy a VGPR each
__device__ inline float uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline double uni(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ inline bool same_bits(double x, double y) { return __double_as_longlong(x) == __double_as_longlong(y); }

// The key of the frame this call leaves behind (MwArgs::fc_key), stored by the env's writer lane as five 16-byte quads: what a plain
// agent-view frame shows of a world that stays installed — the agent's pose, the carried slot and that entity's pose — and the env's
// epoch, which K1 has advanced by then if this call changed anything else (step_env).
__device__ inline void store_frame_key(const MwArgs &a, int env, double px, double py, double pz, double dir, int carry, uint32_t epoch,
                                       double cx, double cy, double cz, double cdir)
{
    ulonglong2 *k = reinterpret_cast<ulonglong2 *>(a.fc_key + (size_t)env * MW_FC_KEY_WORDS);
    auto bits = [](double v) { return (unsigned long long)__double_as_longlong(v); };
    const bool c = carry >= 0;
    k[0] = make_ulonglong2(bits(px), bits(py));
    k[1] = make_ulonglong2(bits(pz), bits(dir));
    k[2] = make_ulonglong2((unsigned long long)(uint32_t)carry | ((unsigned long long)epoch << 32), c ? bits(cx) : 0ull);
    k[3] = make_ulonglong2(c ? bits(cy) : 0ull, c ? bits(cz) : 0ull);
    k[4] = make_ulonglong2(c ? bits(cdir) : 0ull, 1ull);
}

// ---------------------------------------------------------------- dynamics (f64)

struct StepCtx {
    const MwArgs &a;
    int env, lane, set;
    double px, py, pz, dir;        // agent
    double cam_height;
    int carry;                     // slot the agent carries, -1 none
    int live;                      // slot whose pos/dir live in cpos/cdir this step, -1 none
    double cpos[3], cdir;
};

__device__ inline double ent_pos(const StepCtx &c, int slot, int comp)
{
    if (slot == c.live) return c.cpos[comp];
    return c.a.epos[((size_t)comp * c.a.E + slot) * c.a.N + c.env];
}

__device__ inline double ent_geom(const MwArgs &a, int env, int slot, int k)
{
    return a.egeom[((size_t)k * a.E + slot) * a.N + env];
}

// The reference's sums of radii (radii_sum, mw_radii.h: float32 where a mesh entity takes part), decided by the entity's kind, never
// by its value.
using mw::radii_sum;
__device__ inline bool is_mesh(const MwArgs &a, int env, int slot) { return a.ekind[(size_t)slot * a.N + env] == MW_ENT_MESH; }

// MiniWorldEnv.intersect (miniworld.py:937-963): 0 none, -1 wall, 1+slot entity, 1+E agent.  `radius` is the agent's (self_slot
// -1: a Python float) or the radius of the entity self_slot, which the agent carries.
// Every lane passes the same arguments; segments / entities are spread over the lanes.
__device__ int intersect_wave(const StepCtx &c, int self_slot, double x, double z, double radius)
{
    const MwArgs &a = c.a;
    const double *segs = a.segs + (size_t)c.set * a.max_segs * 4;
    const int ns = a.nsegs[c.set];
    const bool rf32 = self_slot >= 0 && is_mesh(a, c.env, self_slot);
    bool hit = false;
    for (int i = c.lane; i < ns; i += 64) {
        const double sax = segs[i * 4 + 0], saz = segs[i * 4 + 1], sbx = segs[i * 4 + 2], sbz = segs[i * 4 + 3];
        const double abx = sbx - sax, abz = sbz - saz;
        const double apx = x - sax, apz = z - saz;
        const double dap = apx * abx + apz * abz;
        const double dab = abx * abx + abz * abz;
        double t = dap / dab;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double cx = sax + t * abx, cz = saz + t * abz;
        const double dx = cx - x, dz = cz - z;
        hit |= sqrt(dx * dx + dz * dz) < radius;
    }
    if (ballot(hit)) return -1;
    for (int base = 0; base < a.E; base += 64) {
        const int slot = base + c.lane;
        bool h = false;
        const int kind = slot < a.E && slot != self_slot ? a.ekind[(size_t)slot * a.N + c.env] : MW_ENT_NONE;
        if (kind != MW_ENT_NONE) {
            const double dx = ent_pos(c, slot, 0) - x, dz = ent_pos(c, slot, 2) - z;
            h = sqrt(dx * dx + dz * dz) < radii_sum(radius, ent_geom(a, c.env, slot, 7), rf32 || kind == MW_ENT_MESH);
        }
        const uint64_t m = ballot(h);
        if (m) return 1 + base + (__ffsll((unsigned long long)m) - 1);
    }
    if (self_slot >= 0) {
        const double dx = c.px - x, dz = c.pz - z;
        if (sqrt(dx * dx + dz * dz) < radii_sum(radius, a.agent_radius, rf32)) return 1 + a.E;
    }
    return 0;
}

// The same query evaluated by ONE lane for its own env (mw_setup_dense.hip: a wavefront holds several envs, the
// lanes of one env all walk its segments and entities and arrive at the same answer).
__device__ int intersect_lane(const StepCtx &c, int self_slot, double x, double z, double radius)
{
    const MwArgs &a = c.a;
    const double *segs = a.segs + (size_t)c.set * a.max_segs * 4;
    const int ns = a.nsegs[c.set];
    const bool rf32 = self_slot >= 0 && is_mesh(a, c.env, self_slot);
    bool hit = false;
#pragma unroll 2
    for (int i = 0; i < ns; ++i) {      // independent iterations: two divisions / square roots in flight
        const double sax = segs[i * 4 + 0], saz = segs[i * 4 + 1], sbx = segs[i * 4 + 2], sbz = segs[i * 4 + 3];
        const double abx = sbx - sax, abz = sbz - saz;
        const double apx = x - sax, apz = z - saz;
        const double dap = apx * abx + apz * abz;
        const double dab = abx * abx + abz * abz;
        double t = dap / dab;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double cx = sax + t * abx, cz = saz + t * abz;
        const double dx = cx - x, dz = cz - z;
        hit |= sqrt(dx * dx + dz * dz) < radius;
    }
    if (hit) return -1;
    for (int slot = 0; slot < a.E; ++slot) {
        const int kind = a.ekind[(size_t)slot * a.N + c.env];
        if (slot == self_slot || kind == MW_ENT_NONE) continue;
        const double dx = ent_pos(c, slot, 0) - x, dz = ent_pos(c, slot, 2) - z;
        if (sqrt(dx * dx + dz * dz) < radii_sum(radius, ent_geom(a, c.env, slot, 7), rf32 || kind == MW_ENT_MESH)) return 1 + slot;
    }
    if (self_slot >= 0) {
        const double dx = c.px - x, dz = c.pz - z;
        if (sqrt(dx * dx + dz * dz) < radii_sum(radius, a.agent_radius, rf32)) return 1 + a.E;
    }
    return 0;
}

template <bool PER_LANE>
__device__ inline int intersect(const StepCtx &c, int self_slot, double x, double z, double radius)
{
    return PER_LANE ? intersect_lane(c, self_slot, x, z, radius) : intersect_wave(c, self_slot, x, z, radius);
}

// _get_carry_pos (miniworld.py:606-618): agent.radius + ent.radius + max_forward_step, in float32 for a mesh entity
__device__ inline void carry_pos(const StepCtx &c, int slot, double ax, double ay, double az, double dvx,
                                 double dvz, double out[3])
{
    const double dist = radii_sum(c.a.agent_radius, ent_geom(c.a, c.env, slot, 7), c.a.max_forward_step, is_mesh(c.a, c.env, slot));
    out[0] = ax + dvx * 1.05 * dist;
    out[1] = ay + 0.0 * 1.05 * dist;
    out[2] = az + dvz * 1.05 * dist;
    const double y = c.cam_height - ent_geom(c.a, c.env, slot, 8) - 0.3;
    out[1] = out[1] + 1.0 * (y > 0.0 ? y : 0.0);
}

// near(ent) (miniworld.py:965-975): 3D distance agent - entity below ent.radius + agent.radius + 1.1 * max_forward_step (the
// product is formed in double and, for a mesh entity, rounded to float32 before it joins the sum)
__device__ inline bool near_agent(const StepCtx &c, int slot)
{
    const double dx = ent_pos(c, slot, 0) - c.px, dy = ent_pos(c, slot, 1) - c.py, dz = ent_pos(c, slot, 2) - c.pz;
    return sqrt(dx * dx + dy * dy + dz * dz) <
           radii_sum(ent_geom(c.a, c.env, slot, 7), c.a.agent_radius, 1.1 * c.a.max_forward_step, is_mesh(c.a, c.env, slot));
}

// The env rules that live in the placement program's tables (include/mwengine.h):
// Sidewalk.step (sidewalk.py:93-104): the street ends the episode and zeroes the reward, the box adds the GOTO reward;
// Sign.step (sign.py:152-170): action move_forward + 1 ends the episode, touching an object ends it with +-1.
__device__ inline void program_rules(const StepCtx &c, int action, int step_count, double &rew, int &tm)
{
    const MwArgs &a = c.a;
    if (a.task == MW_TASK_SIDEWALK) {
        const double *st = a.prog->p.street;
        if (c.px > st[0] && c.px < st[1] && c.pz > st[2] && c.pz < st[3]) { rew = 0.0; tm = 1; }     // Room.point_inside
        if (near_agent(c, a.goal_ent)) {
            rew += 1.0 - 0.2 * ((double)step_count / (double)a.max_steps);
            tm = 1;
        }
    } else if (a.task == MW_TASK_SIGN) {
        if (action == 3) tm = 1;                    // actions.move_forward + 1: the custom end-of-episode action
        const mw_gen_program &g = a.prog->p;
        for (int k = 0; k < g.sign_n; ++k)
            if (near_agent(c, g.sign_slot[k])) { tm = 1; rew = g.sign_reward[k]; }
    }
}

template <bool PER_LANE>
__device__ void move_agent(StepCtx &c, double fwd_dist, double fwd_drift)
{
    const mw::SinCos sc = mw::sincos_det(c.dir);
    const double dvx = sc.c, dvz = -sc.s, rvx = sc.s, rvz = sc.c;
    const double nx = c.px + dvx * fwd_dist + rvx * fwd_drift;
    const double ny = c.py + 0.0 * fwd_dist + 0.0 * fwd_drift;
    const double nz = c.pz + dvz * fwd_dist + rvz * fwd_drift;
    if (intersect<PER_LANE>(c, -1, nx, nz, c.a.agent_radius)) return;
    if (c.carry >= 0) {
        double cp[3];
        carry_pos(c, c.carry, nx, ny, nz, dvx, dvz, cp);
        if (intersect<PER_LANE>(c, c.carry, cp[0], cp[2], ent_geom(c.a, c.env, c.carry, 7))) return;
        c.cpos[0] = cp[0]; c.cpos[1] = cp[1]; c.cpos[2] = cp[2];
    }
    c.px = nx; c.py = ny; c.pz = nz;
}

template <bool PER_LANE>
__device__ void turn_agent(StepCtx &c, double turn_deg)
{
    const double turn = turn_deg * (kPi / 180.0);
    const double orig = c.dir;
    c.dir = c.dir + turn;
    if (c.carry >= 0) {
        const mw::SinCos sc = mw::sincos_det(c.dir);
        double cp[3];
        carry_pos(c, c.carry, c.px, c.py, c.pz, sc.c, -sc.s, cp);
        if (intersect<PER_LANE>(c, c.carry, cp[0], cp[2], ent_geom(c.a, c.env, c.carry, 7))) {
            c.dir = orig;
            return;
        }
        c.cpos[0] = cp[0]; c.cpos[1] = cp[1]; c.cpos[2] = cp[2];
        c.cdir = c.dir;
    }
}

// What one sub-step hands to the loop of a repeat call (step_env_repeat); the plain step ignores it.
struct SubStep {
    double rew;             // the sub-step's reward, before it is rounded to float
    int tm, tr;
    int remove_slot;        // what the sub-step left in pending_remove
    bool ran;               // false: the call installed a pending next-step reset instead of stepping
    bool clean;             // the writer lane's frame_clean value of this sub-step
};

// TRACE (mw_step_plan_trace's kernels, MW_K1_MODE 3): row `row` of env `env` in the caller's trace arrays (mw_plan_trace,
// mwengine.h: [horizon][N] rows in mw_state_view's row layout, any field may be null) := the agent's pose, the carried slot as the
// step stores it and the position of slot ent_slot — from the writer lane's registers where the step has them (`live`: the slot whose
// position is in cpos, or -1), else from the engine's arrays.
__device__ inline void trace_store(const MwArgs &a, const mw_plan_trace &t, int row, int env, double px, double py, double pz, double dir, int carry,
                                   int live, const double *cpos)
{
    const size_t r = (size_t)row * a.N + env;
    if (t.agent_pos) { t.agent_pos[r * 3 + 0] = px; t.agent_pos[r * 3 + 1] = py; t.agent_pos[r * 3 + 2] = pz; }
    if (t.agent_dir) t.agent_dir[r] = dir;
    if (t.carrying) t.carrying[r] = carry;
    if (t.ent_pos) {
        const int s = t.ent_slot;
        const bool held = live == s;
        t.ent_pos[r * 3 + 0] = held ? cpos[0] : a.epos[((size_t)0 * a.E + s) * a.N + env];
        t.ent_pos[r * 3 + 1] = held ? cpos[1] : a.epos[((size_t)1 * a.E + s) * a.N + env];
        t.ent_pos[r * 3 + 2] = held ? cpos[2] : a.epos[((size_t)2 * a.E + s) * a.N + env];
    }
}
// ... and rows k0 .. k1 - 1 := row src: the rows of the sub-steps an env did not execute repeat the state it stopped in
__device__ inline void trace_fill(const MwArgs &a, const mw_plan_trace &t, int src, int k0, int k1, int env)
{
    if (k0 >= k1) return;
    const size_t N = (size_t)a.N, s = (size_t)src * N + env;
    if (t.agent_pos) {
        const double x = t.agent_pos[s * 3 + 0], y = t.agent_pos[s * 3 + 1], z = t.agent_pos[s * 3 + 2];
        for (int k = k0; k < k1; ++k) { double *d = t.agent_pos + ((size_t)k * N + env) * 3; d[0] = x; d[1] = y; d[2] = z; }
    }
    if (t.agent_dir) {
        const double v = t.agent_dir[s];
        for (int k = k0; k < k1; ++k) t.agent_dir[(size_t)k * N + env] = v;
    }
    if (t.carrying) {
        const int32_t v = t.carrying[s];
        for (int k = k0; k < k1; ++k) t.carrying[(size_t)k * N + env] = v;
    }
    if (t.ent_pos) {
        const double x = t.ent_pos[s * 3 + 0], y = t.ent_pos[s * 3 + 1], z = t.ent_pos[s * 3 + 2];
        for (int k = k0; k < k1; ++k) { double *d = t.ent_pos + ((size_t)k * N + env) * 3; d[0] = x; d[1] = y; d[2] = z; }
    }
}

// One env's step, the body of both K1 forms (mw_setup.hip: one wavefront per env, PER_LANE = false, the 64 lanes share the
// collision tests; mw_setup_dense.hip: several envs per wavefront, PER_LANE = true, each lane tests alone).  Every lane of the
// env calls it with the same env and evaluates the step; `writer`, one lane of the env, writes its state and flags.
// Replaces, per env and per step (reference file:line):
//   MiniWorldEnv.step / move_agent / turn_agent / _get_carry_pos   miniworld.py:606-730
//   MiniWorldEnv.intersect + intersect_circle_segs                 miniworld.py:937-963, math.py:30-62
//   near / _reward + env rules                                     miniworld.py:965-975,1012-1017; hallway.py:67-74; pickupobjects.py:83-95
// The frame itself — camera, transform, lighting, clipping, triangle setup — is the geometry kernel's (mw_geom.hip).
// REPEAT: one sub-step of mw_step_repeat — the same step, except that reward, flags and the frame_clean byte are the loop's to
// write, once per call (step_env_repeat).
// TRACE: the writer lane also stores row trace_row of the caller's trace (trace_store) beside the env's state — the state the sub-step
// leaves, before the install site below replaces it with the next episode's; for a pending next-step reset, the state the call found.
// A compile-time constant like REPEAT: the two arguments behind it do not exist in the kernels that leave it false.
template <bool PER_LANE, bool REPEAT = false, bool TRACE = false>
__device__ inline SubStep step_env(const MwArgs &a, int env, int lane, bool writer, const int32_t *__restrict__ actions,
                                float *__restrict__ reward, uint8_t *__restrict__ term, uint8_t *__restrict__ trunc,
                                unsigned char *gen_ws, int *s_claim, const mw_plan_trace *trace = nullptr, int trace_row = 0)
{
    StepCtx c{a, env, lane, a.shared_geom ? 0 : env, 0, 0, 0, 0, 0, -1, -1, {0, 0, 0}, 0};
    c.px = a.ax[env]; c.py = a.ay[env]; c.pz = a.az[env]; c.dir = a.adir[env];
    c.cam_height = a.cam[env];
    c.carry = a.carry[env];
    if (c.carry >= 0) {
        const int k = c.carry;
        c.cpos[0] = ent_pos(c, k, 0); c.cpos[1] = ent_pos(c, k, 1); c.cpos[2] = ent_pos(c, k, 2);
        c.cdir = a.edir[(size_t)k * a.N + env];
        c.live = k;
    }
    // the state as loaded, for the frame_clean byte: what the frame shows of an env is its agent's pose and its entities'
    const double o_px = c.px, o_py = c.py, o_pz = c.pz, o_dir = c.dir, o_cpos[3] = {c.cpos[0], c.cpos[1], c.cpos[2]}, o_cdir = c.cdir;
    const int o_carry = c.carry;
    const int o_pending = a.pending_remove[env];        // (what the last step left; -1: nothing left or has just left the list)
    const uint32_t o_epoch = a.fc_epoch[env];
    bool same = false;              // the state this step stores is the state it loaded, bit for bit
    int remove_slot = -1;
    int tm = 0, tr = 0;             // terminated / truncated, uniform over the env's lanes
    double rew_out = 0.0;
    bool clean_out = false;
    // next-step auto-reset: the env's last step ended its episode (and drew its terminal state); this step installs the
    // next world instead of stepping — no action, no per-step draws (miniworld.py:677-680 are step()'s, not reset()'s)
    const bool pend = a.autoreset == MW_AUTORESET_NEXT_STEP && a.reset_pending[env] != 0;

    if (!pend) {
        const int step_count = a.step[env] + 1;
        int picked = a.picked[env];
        // the three per-step parameters (miniworld.py:677-680)
        double fwd_step = a.fwd.def, fwd_drift = a.drift.def, turn_step = a.turn.def;
        mw::Rng rng{};
        bool drew = false;
        if (a.step_override) {
            fwd_step = a.step_override[(size_t)env * 3 + 0];
            fwd_drift = a.step_override[(size_t)env * 3 + 1];
            turn_step = a.step_override[(size_t)env * 3 + 2];
        } else if (a.domain_rand) {
            rng = mw::rng_load(a.rng, a.N, env);
            fwd_step = mw::rng_uniform(rng, a.fwd.lo, a.fwd.hi);
            fwd_drift = mw::rng_uniform(rng, a.drift.lo, a.drift.hi);
            turn_step = mw::rng_uniform(rng, a.turn.lo, a.turn.hi);
            drew = true;            // stored with the rest of the state, below
        }
        const int action = actions[env];
        switch (action) {
        case 2: move_agent<PER_LANE>(c, fwd_step, fwd_drift); break;
        case 3: move_agent<PER_LANE>(c, -fwd_step, fwd_drift); break;
        case 0: turn_agent<PER_LANE>(c, turn_step); break;
        case 1: turn_agent<PER_LANE>(c, -turn_step); break;
        case 4: {   // pickup (miniworld.py:695-702)
            const mw::SinCos sc = mw::sincos_det(c.dir);
            const double tx = c.px + sc.c * 1.5 * a.agent_radius;
            const double tz = c.pz + (-sc.s) * 1.5 * a.agent_radius;
            const int hit = intersect<PER_LANE>(c, -1, tx, tz, 1.2 * a.agent_radius);
            if (c.carry < 0 && hit > 0 && hit <= a.E && !a.estatic[(size_t)(hit - 1) * a.N + env]) {
                const int k = hit - 1;
                c.cpos[0] = ent_pos(c, k, 0); c.cpos[1] = ent_pos(c, k, 1); c.cpos[2] = ent_pos(c, k, 2);
                c.cdir = a.edir[(size_t)k * a.N + env];
                c.carry = k;
                c.live = k;
            }
            break;
        }
        case 5:     // drop (miniworld.py:705-708)
            if (c.carry >= 0) {
                c.cpos[1] = 0.0;
                c.carry = -1;       // the live copy is written back at the end of the step
            }
            break;
        default: break;
        }
        if (c.carry >= 0) {     // carried object follows (miniworld.py:711-714)
            const mw::SinCos sc = mw::sincos_det(c.dir);
            double cp[3];
            carry_pos(c, c.carry, c.px, c.py, c.pz, sc.c, -sc.s, cp);
            c.cpos[0] = cp[0]; c.cpos[1] = cp[1]; c.cpos[2] = cp[2];
            c.cdir = c.dir;
        }
        // reward / termination (miniworld.py:720-730 + env rule)
        double rew = 0.0;
        tr = step_count >= a.max_steps ? 1 : 0;
        if (a.task == MW_TASK_GOTO) {
            if (near_agent(c, a.goal_ent)) {
                rew += 1.0 - 0.2 * ((double)step_count / (double)a.max_steps);
                tm = 1;
            }
        } else if (a.task == MW_TASK_PUTNEXT) {
            if (c.carry < 0) {      // putnext.py:74-78
                const int g0 = a.goal_ent, g1 = a.goal_ent2;
                const double dx = ent_pos(c, g0, 0) - ent_pos(c, g1, 0), dy = ent_pos(c, g0, 1) - ent_pos(c, g1, 1),
                             dz = ent_pos(c, g0, 2) - ent_pos(c, g1, 2);
                const double dist = sqrt(dx * dx + dy * dy + dz * dz);
                if (dist < radii_sum(ent_geom(a, env, g0, 7), ent_geom(a, env, g1, 7), 1.1 * a.max_forward_step, is_mesh(a, env, g0) || is_mesh(a, env, g1))) {
                    rew += 1.0 - 0.2 * ((double)step_count / (double)a.max_steps);
                    tm = 1;
                }
            }
        } else if (a.task == MW_TASK_PICKUP) {
            if (c.carry >= 0) {
                remove_slot = c.carry;      // still drawn this frame (pickupobjects.py:86-88 runs after :717)
                picked += 1;
                rew = 1.0;
                if (picked == a.num_objs) tm = 1;
            }
        }
        if (a.task >= MW_TASK_SIDEWALK) program_rules(c, action, step_count, rew, tm);
        // CollectHealth (collecthealth.py:79-98) never takes the dense form (mw_policy.h: k1_dense_lanes)
        int health = 0;
        if (!PER_LANE && a.task == MW_TASK_COLLECT) {
            health = a.health[env] - 2;
            if (action == 4 && c.carry >= 0) {  // the kit in hand is consumed — after this frame was drawn (remove_slot)
                remove_slot = c.carry;
                health = 100;
            }
            if (health > 0) rew = 2.0; else { rew = -100.0; tm = 1; }
        }
        if (REPEAT) rew_out = rew;
        // (compared, not tracked through the code paths above: a blocked move, a turn a carried box undoes, a pickup that finds
        // nothing all end here with the loaded values; a slot that is live now and was not carried before fails on `carry`)
        same = same_bits(c.px, o_px) && same_bits(c.py, o_py) && same_bits(c.pz, o_pz) && same_bits(c.dir, o_dir) && c.carry == o_carry &&
               (c.live < 0 || (same_bits(c.cpos[0], o_cpos[0]) && same_bits(c.cpos[1], o_cpos[1]) && same_bits(c.cpos[2], o_cpos[2]) && same_bits(c.cdir, o_cdir)));
        // every lane of the env has read the old state (the lanes of a wavefront run in lockstep, and each lane only reads its
        // own env's): the writer stores the new one
        if (PER_LANE) __builtin_amdgcn_wave_barrier();
        if (writer) {
            if (drew) mw::rng_store(a.rng, a.N, env, rng);
            if (!REPEAT) {
                reward[env] = (float)rew;
                term[env] = (uint8_t)tm;
                trunc[env] = (uint8_t)tr;
            }
            a.step[env] = step_count;
            a.picked[env] = picked;
            if (!PER_LANE && a.task == MW_TASK_COLLECT) a.health[env] = health;
            // agent + carried entity
            a.ax[env] = c.px; a.ay[env] = c.py; a.az[env] = c.pz; a.adir[env] = c.dir;
            if (c.live >= 0) {
                a.epos[((size_t)0 * a.E + c.live) * a.N + env] = c.cpos[0];
                a.epos[((size_t)1 * a.E + c.live) * a.N + env] = c.cpos[1];
                a.epos[((size_t)2 * a.E + c.live) * a.N + env] = c.cpos[2];
                a.edir[(size_t)c.live * a.N + env] = c.cdir;
            }
            a.carry[env] = remove_slot >= 0 ? -1 : c.carry;
            if (TRACE) trace_store(a, *trace, trace_row, env, c.px, c.py, c.pz, c.dir, remove_slot >= 0 ? -1 : c.carry, c.live, c.cpos);
            if ((tm | tr) && a.autoreset != MW_AUTORESET_OFF && a.generator != MW_GEN_NONE) {
                mw::keep_final_info(a, env);
                if (a.autoreset == MW_AUTORESET_NEXT_STEP) a.reset_pending[env] = 1;
            }
        }
    } else if (writer && !REPEAT) {
        reward[env] = 0.0f;
        term[env] = 0;
        trunc[env] = 0;
    } else if (TRACE && writer) {
        trace_store(a, *trace, trace_row, env, c.px, c.py, c.pz, c.dir, c.carry, c.live, c.cpos);
    }
    // The one install site of the next world.  Same-step auto-reset: on the step that ends the episode, so that the observation
    // returned with done = 1 is the first one of the next episode.  Next-step auto-reset: on the step after it, the reference's
    // "step; if done: reset()" (scripts/benchmark.py:36-37) — the stream is consumed in that order.
    bool installed = false;
    if (a.generator != MW_GEN_NONE && (pend || (a.autoreset == MW_AUTORESET_SAME_STEP && (tm | tr)))) {
        installed = true;
        if (PER_LANE) {
            // the env's leading lane installs it (several envs of the wave may do so side by side); the env's other lanes then
            // read it like the leader does
            if (writer) mw::install_next_world<true>(a, env, 0, gen_ws, nullptr);
            __threadfence();
            __builtin_amdgcn_wave_barrier();
        } else {
            mw::install_next_world<false>(a, env, lane, gen_ws, s_claim);
        }
        c.px = a.ax[env]; c.py = a.ay[env]; c.pz = a.az[env]; c.dir = a.adir[env];
        c.carry = -1; c.live = -1;
        remove_slot = -1;
        if (pend && writer) a.reset_pending[env] = 0;
    }

    // what this step leaves for after its frame (a picked-up object is drawn one last time, pickupobjects.py:86-88) goes with
    // the frame's vertex half, mw_geom_kernel's (mw_geom.hip)
    if (writer) {
        // frame_clean: the frame after this step is the frame before it.  Not when an entity leaves the list behind this frame or
        // left it behind the last one (the geometry kernel applied that removal after the last frame was drawn: MW_REMOVE_APPLIED;
        // a slot still pending was never applied), not on a next-step reset, not when a world was installed.  CollectHealth never:
        // its respawn kernel moves entities behind this kernel's back.
        const bool clean = same && !pend && !installed && remove_slot < 0 && o_pending == -1 && a.task != MW_TASK_COLLECT;
        if (REPEAT) clean_out = clean; else { a.frame_clean[env] = clean ? 1 : 0; a.fc_source[env] = 0; }
        // the frame cache's epoch: everything that forces clean = 0 whatever the poses say also parts the frames before it from the
        // frames after it — a world installed, a removal the geometry kernel applied behind the last frame (the frame of the step
        // that removes still shows the entity), a change of the carried slot (a dropped entity stays where it was put)
        const bool parted = pend || installed || o_pending != -1 || c.carry != o_carry;
        if (parted) a.fc_epoch[env] = o_epoch + 1u;
        if (!REPEAT) store_frame_key(a, env, c.px, c.py, c.pz, c.dir, c.carry, o_epoch + (parted ? 1u : 0u), c.cpos[0], c.cpos[1], c.cpos[2], c.cdir);
        a.pending_remove[env] = remove_slot;
    }
    return SubStep{rew_out, tm, tr, remove_slot, !pend, clean_out};
}

// mw_step_repeat's step of one env: up to `repeat` sub-steps with the same action, each one step_env, until one ends the episode;
// the auto-reset (step_env's one install site) runs on that sub-step, or instead of the first one for a pending next-step reset,
// so an env never steps in two episodes within one call.  Between two sub-steps the writer lane applies what the frame's tail
// applies after a rendered step: a picked-up object leaves the list (pickupobjects.py:86-88 — the geometry kernel's part),
// CollectHealth's consumed kit respawns with its draws from the env's stream (mw_collect_respawn_kernel's part).  The last
// executed sub-step's removal stays in pending_remove for those two, so the object is drawn one last time.  The reward is summed
// in double, in order, and rounded once; flags are the last executed sub-step's; frame_clean: at least one sub-step ran and every
// one left the state as it was.
// The envs of a dense wavefront stop at different sub-steps: the trip count is the wavefront's — the loop ends when none of its
// envs is active — and an env that has stopped is predicated off, its lanes stay in the loop.
//
// PLAN: mw_step_plan's step of one env — the same loop with the action of sub-step k read from row k of `actions` ([repeat][N],
// sub-step-major: the envs of a dense wavefront read consecutive words) and the float reward a single mw_step would have returned for
// sub-step k stored to step_reward[k][env] (may be null), 0 for every sub-step the env did not execute.  `frameless`: no frame follows
// the call, so the writer lane applies the frame's tail behind the LAST executed sub-step too — whatever the geometry kernel and
// the respawn kernel of a drawn call would have found in pending_remove: nothing where that sub-step installed a world (step_env
// leaves -1 there), the removal or the respawn on a terminal sub-step that installed none — and frame_clean is 0.  Both arguments are
// compile-time constants of the repeat kernels, whose code they leave as it was.
//
// TRACE (with PLAN): mw_step_plan_trace's — every executed sub-step stores its row of `trace` (step_env), and so does the sub-step that
// found a pending next-step reset; the rows behind an env's last one, inside the loop where other envs of the wavefront are still
// stepping and behind it, repeat that row (the pattern of step_reward's zero fill).  A compile-time constant of the repeat and plan
// kernels, whose code it leaves as it was.
template <bool PER_LANE, bool PLAN = false, bool TRACE = false>
__device__ inline void step_env_repeat(const MwArgs &a, int env, int lane, bool writer, const int32_t *__restrict__ actions, int repeat,
                                       float *__restrict__ reward, uint8_t *__restrict__ term, uint8_t *__restrict__ trunc,
                                       int32_t *__restrict__ nsteps, float *__restrict__ step_reward, bool frameless, unsigned char *gen_ws,
                                       int *s_claim, const mw_plan_trace *trace = nullptr)
{
    double sum = 0.0;
    int n = 0, tm = 0, tr = 0;
    bool clean = true, active = true;
    int rows = 0;           // PLAN: the rows of step_reward the loop has written (the wavefront's trip count)
    for (int k = 0; k < repeat; ++k) {
        if (!ballot(active)) break;
        float rew_k = 0.0f;
        if (active) {
            const SubStep s = step_env<PER_LANE, true, TRACE>(a, env, lane, writer, PLAN ? actions + (size_t)k * a.N : actions, reward, term, trunc, gen_ws, s_claim,
                                                              trace, k);
            if (s.ran) {
                sum += s.rew;
                ++n;
                tm = s.tm; tr = s.tr;
                clean = clean && s.clean;
                if (PLAN) rew_k = (float)s.rew;
            }
            active = s.ran && !(tm | tr) && k + 1 < repeat;
            if ((active || (PLAN && frameless)) && writer && s.remove_slot >= 0) {
                if (a.task == MW_TASK_COLLECT) {
                    mw::collect_respawn(a, env, a.shared_geom ? 0 : env, s.remove_slot, a.ax[env], a.az[env]);
                    a.pending_remove[env] = -1;
                } else {
                    a.ekind[(size_t)s.remove_slot * a.N + env] = MW_ENT_NONE;
                    a.pending_remove[env] = MW_REMOVE_APPLIED;
                }
            }
        } else if (TRACE && writer) {
            trace_fill(a, *trace, k - 1, k, k + 1, env);        // (an env is active at k = 0)
        }
        if (PLAN) {
            if (writer && step_reward) step_reward[(size_t)k * a.N + env] = rew_k;
            rows = k + 1;
        }
        // the env's lanes reload its state for the next sub-step: after the writer's stores (the install site's pattern, at
        // workgroup scope: the lanes that reload are the writer's own wavefront, which is the whole workgroup in both forms.  The
        // device-scope __threadfence() here, an L2 write-back and invalidate per sub-step, made the dense kernel 118 us at
        // K = 4 where this one takes 48)
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
    }
    if (writer) {
        if (PLAN && step_reward)
            for (int k = rows; k < repeat; ++k) step_reward[(size_t)k * a.N + env] = 0.0f;
        if (TRACE) trace_fill(a, *trace, rows - 1, rows, repeat, env);
        reward[env] = (float)sum;
        term[env] = (uint8_t)tm;
        trunc[env] = (uint8_t)tr;
        if (nsteps) nsteps[env] = n;
        a.frame_clean[env] = !(PLAN && frameless) && n > 0 && clean ? 1 : 0;
        a.fc_source[env] = 0;
        // the key of the state the last sub-step left, once per call, from the writer's own stores: the slot the frame shows as
        // carried is the one that leaves the list behind it, if any (step_env: remove_slot), else the carried one
        const int pr = a.pending_remove[env], k = pr >= 0 ? pr : a.carry[env], ks = k >= 0 ? k : 0;
        store_frame_key(a, env, a.ax[env], a.ay[env], a.az[env], a.adir[env], k, a.fc_epoch[env], a.epos[((size_t)0 * a.E + ks) * a.N + env],
                        a.epos[((size_t)1 * a.E + ks) * a.N + env], a.epos[((size_t)2 * a.E + ks) * a.N + env], a.edir[(size_t)ks * a.N + env]);
    }
}

}  // namespace

// The two K1 sources (mw_setup.hip, mw_setup_dense.hip) compile once per mode of mw_kernels.h's table, MW_K1_MODE (the Makefile sets
// it): the row of the mode gives the kernel's stem and parameters, the branch here its call of the step body — the same grid mapping
// and refill blocks around it in every mode.
//   0  the plain step
//   1  mw_step_repeat's: the sub-step loop, `repeat` and `nsteps` as two more kernel parameters
//   2  mw_step_plan's: the loop with PLAN set, `actions` the [horizon][N] plans
//   3  mw_step_plan_trace's: TRACE set too, the caller's trace one more parameter
#ifndef MW_K1_MODE
#define MW_K1_MODE 0
#endif
#define MW_K1_ROW MW_CAT(MW_K1_ROW_, MW_K1_MODE)
#define MW_K1_PARAMS MW_K1_ROW(MW_K1_PARAMS_OF)
#define MW_K1_NAME(form) MW_KERNEL_NAME(MW_CAT(MW_K1_ROW(MW_K1_STEM), form))      // form: empty (wave per env) or _dense
#if MW_K1_MODE == 0
#define MW_K1_STEP(PER_LANE, env, lane, writer, ws, claim) step_env<PER_LANE>(a, env, lane, writer, actions, reward, term, trunc, ws, claim)
#elif MW_K1_MODE == 1
#define MW_K1_STEP(PER_LANE, env, lane, writer, ws, claim) \
    step_env_repeat<PER_LANE>(a, env, lane, writer, actions, repeat, reward, term, trunc, nsteps, nullptr, false, ws, claim)
#elif MW_K1_MODE == 2
#define MW_K1_STEP(PER_LANE, env, lane, writer, ws, claim) \
    step_env_repeat<PER_LANE, true>(a, env, lane, writer, actions, horizon, reward, term, trunc, nsteps, step_reward, frameless != 0, ws, claim)
#elif MW_K1_MODE == 3
#define MW_K1_STEP(PER_LANE, env, lane, writer, ws, claim) \
    step_env_repeat<PER_LANE, true, true>(a, env, lane, writer, actions, horizon, reward, term, trunc, nsteps, step_reward, frameless != 0, ws, claim, &trace)
#else
#error "MW_K1_MODE is not a mode of mw_kernels.h's K1 table"
#endif
