/* mwengine — C ABI of the MI355X-native batched Miniworld step+render engine.
 *
 * The reference (Farama-Foundation/Miniworld v2.1.0) has no FFI: its "backend" is the
 * Python module miniworld/opengl.py (Texture, FrameBuffer, drawBox) plus raw GL calls in
 * Entity.render(), driven once per MiniWorldEnv.step().  This header is the seam a
 * maintainer binds instead of that module (ctypes stub: INTEGRATION.md).  Every entry
 * point cites the reference interface it replaces.
 *
 * Conventions
 *   - plain C, no exceptions: every call returns 0 on success or a negative MW_E_* code;
 *     mw_last_error() gives the message (reference: Python assert / exception).
 *   - the CALLER owns all output buffers (device pointers, e.g. torch tensors); the engine
 *     owns the Structure-of-Arrays world state of its N environments.
 *   - all device work is enqueued on the hipStream_t passed as `stream` (void* so that this
 *     header needs no HIP include); nothing synchronises unless documented.
 *   - one engine per device; an engine is not re-entrant (the reference is single-threaded:
 *     one GL context per env, miniworld.py:1187), distinct engines are independent.
 */
#ifndef MWENGINE_H
#define MWENGINE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MW_ABI_VERSION 4

enum {
    MW_OK = 0,
    MW_E_INVALID = -1,      /* bad argument                                 */
    MW_E_HIP = -2,          /* HIP runtime error (message has the hipError) */
    MW_E_NOMEM = -3,
    MW_E_CAPACITY = -4,     /* more polys / entities / textures than configured */
    MW_E_DEVICE = -5,       /* no usable gfx950 device                      */
    MW_E_OVERFLOW = -6      /* a kernel reported a per-env capacity overflow */
};

/* entity kinds (entity.py: Box :386, MeshEnt :124 / Ball :445 / Key :435, ImageFrame :168 / TextFrame :262).
 * MW_ENT_FRAME: the entity's quads are part of the static polygon list (mw_set_geometry) — it is an entity
 * only for collisions (radius 0, miniworld.py:951-961) and for mw_visible_ents. */
enum { MW_ENT_NONE = 0, MW_ENT_BOX = 1, MW_ENT_MESH = 2, MW_ENT_FRAME = 3 };

/* env reward / termination rule applied after MiniWorldEnv.step (miniworld.py:670-730) */
enum {
    MW_TASK_NONE = 0,
    MW_TASK_GOTO = 1,       /* hallway.py:67-74, oneroom.py:64-71, maze.py:155-162 */
    MW_TASK_PICKUP = 2,     /* pickupobjects.py:83-95                            */
    MW_TASK_PUTNEXT = 3,    /* putnext.py:71-80: goal_ent next to goal_ent2, not carrying */
    MW_TASK_SIDEWALK = 4,   /* sidewalk.py:93-104: the street ends the episode with reward 0, the box like GOTO
                             * (mw_gen_program.street, goal_ent) */
    MW_TASK_SIGN = 5,       /* sign.py:152-170: action move_forward + 1 ends the episode; touching an object of the
                             * table ends it with +-1, the last one touched wins (mw_gen_program.sign_*) */
    MW_TASK_COLLECT = 6     /* collecthealth.py:79-98: health -2 per step, +2 reward while alive, -100 and the end at 0;
                             * a kit picked up is consumed after the frame was drawn: health back to 100, the kit leaves
                             * the entity list and is re-placed at its END with the env's own stream (place_entity) */
};

/* device-side world generators for mw_reset / auto-reset (the env's _gen_world) */
enum {
    MW_GEN_NONE = 0,        /* worlds only come from mw_set_state             */
    MW_GEN_HALLWAY = 1,     /* hallway.py:55-65                               */
    MW_GEN_ONEROOM = 2,     /* oneroom.py:59-62                               */
    MW_GEN_PICKUP = 3,      /* pickupobjects.py:55-81                         */
    MW_GEN_MAZE = 4,        /* maze.py:73-153 (needs shared_geometry = 0)     */
    MW_GEN_PROGRAM = 5      /* a fixed floorplan whose _gen_world is a list of draws and placements: the placement
                             * program of mw_set_gen_program (FourRooms, TMaze*, YMaze*, WallGap, ThreeRooms, PutNext,
                             * RoomObjects, Sidewalk, Sign, ...) */
};

/* Random stream of device-side resets.  MW_RNG_PHILOX: Philox4x32-10 keyed by the env's seed (same
 * distributions as the reference, different numbers; every generator, with or without domain
 * randomisation).  MW_RNG_PCG64: numpy's Generator(PCG64(SeedSequence(seed))) itself, drawn in the
 * reference's call order (miniworld.py:551, 872-905; hallway.py:59-65, oneroom.py:61-62), so that env i
 * reset with seed s is the world of the reference's env.reset(seed=s), and later episodes continue that
 * stream like env.reset() does (with domain randomisation the per-step parameters come from it too,
 * miniworld.py:677-680).  Every device generator, with and without domain_rand (the Maze's room textures exist in one
 * variant each in the reference, so Room._gen_static_data's variant draws consume nothing there, opengl.py:134-138). */
enum { MW_RNG_PHILOX = 0, MW_RNG_PCG64 = 1 };
/* Auto-reset of the envs whose episode ended (term | trunc), on the device, with the configured generator (none with MW_GEN_NONE):
 *   MW_AUTORESET_OFF        never: the caller resets with mw_reset(mask, ...).
 *   MW_AUTORESET_SAME_STEP  the step that ends an episode installs the next world before its frame is drawn: the observation returned
 *                           with done = 1 is the first one of the next episode (the terminal frame is never drawn).
 *   MW_AUTORESET_NEXT_STEP  the step that ends an episode is an ordinary step (its frame shows the terminal state, its reward and flags
 *                           are the episode's last); the env's NEXT step ignores its action, installs the next world and returns that
 *                           world's first frame with reward 0 and term = trunc = 0.  The reference's "step; if done: reset()", stream
 *                           order included (Gymnasium's AutoresetMode.NEXT_STEP); mw_get_reset_pending tells which envs such a
 *                           step will reset. */
enum { MW_AUTORESET_OFF = 0, MW_AUTORESET_SAME_STEP = 1, MW_AUTORESET_NEXT_STEP = 2 };

typedef struct mw_engine mw_engine;

/* Scalar simulation parameter with its domain-randomisation range (params.py:7-130). */
typedef struct { double def, lo, hi; } mw_range;

typedef struct {
    int32_t abi_version;        /* MW_ABI_VERSION */
    int32_t device_id;
    int32_t num_envs;
    int32_t obs_width, obs_height;  /* MiniWorldEnv(obs_width=80, obs_height=60) miniworld.py:473-474: any size from 1 x 1 to
                                     * 4080 x 1020.  Frames that are not multiples of the 16 x 4 raster tile (84 x 84,
                                     * 81 x 61, ...) take the ragged tile kernels or the generic-resolution kernels
                                     * (mw_raster_path)                                                               */
    int32_t msaa;               /* FrameBuffer(..., num_samples=8) miniworld.py:515.  8 = the hot path; 4 or 1 = what the
                                 * reference falls back to on a driver that clamps GL_MAX_SAMPLES (opengl.py:229-231):
                                 * same semantics through the generic-resolution kernels, every obs layout            */
    int32_t max_ents;           /* entity slots per env, agent excluded            */
    int32_t max_polys;          /* room polygons per geometry set                  */
    int32_t max_segs;           /* collision segments per geometry set             */
    int32_t max_visible;        /* GL primitives (polygons, box faces) that can be in view per env: the triangle list holds 6 x this (two triangles per primitive, three pieces each after clipping — a heuristic: a triangle across the near plane and two side planes clips to four or five pieces, back-face culling halves the list; mw_get_list_lengths reports what a workload needs).  A longer list is an error of mw_check, never a write out of bounds */
    int32_t shared_geometry;    /* 1: one geometry set for all envs, 0: one per env */
    int32_t task;               /* MW_TASK_*                                       */
    int32_t goal_ent;           /* MW_TASK_GOTO: entity slot of the box            */
    int32_t goal_ent2;          /* MW_TASK_PUTNEXT: slot of the second entity      */
    int32_t num_objs;           /* MW_TASK_PICKUP                                  */
    int32_t max_episode_steps;  /* miniworld.py:472, per env class                 */
    int32_t domain_rand;        /* miniworld.py:478                                */
    int32_t generator;          /* MW_GEN_*                                        */
    int32_t autoreset;          /* MW_AUTORESET_* (mw_create rejects other values)  */
    double agent_radius;        /* entity.py:470 (0.4)                             */
    double agent_height;        /* entity.py:471 (1.6): height of the top-view marker */
    double max_forward_step;    /* params.get_max("forward_step") miniworld.py:581 */
    mw_range forward_step, forward_drift, turn_step;   /* params.py:123-125, miniworld.py:678-680 */
    /* per-episode parameters sampled by reset (miniworld.py:576-585, entity.py:405-407, 505-515) */
    mw_range sky_color[3], light_pos[3], light_color[3], light_ambient[3];   /* params.py:116-121 */
    mw_range obj_color_bias[3];                                               /* params.py:122     */
    mw_range cam_height, cam_fwd_disp, cam_pitch, cam_fov_y;                  /* params.py:127-130 */
    /* generator parameters: [0..3] room min_x,max_x,min_z,max_z; [4] box min_x override;
     * [5] agent max_x override; [6] agent |dir| range; [7] box size */
    double gen_args[8];
    /* MW_GEN_PICKUP: per object kind (Ball, Box, Key — pickupobjects.py:65): radius, height, scale,
     * first mesh id (mesh ids of one kind are consecutive in sorted colour order); and the RGB of the
     * six colours in sorted name order (entity.py:30-43) */
    double gen_tab[12];
    double gen_colors[18];
    /* Texture domain randomisation for generated single-room worlds (Texture.get with an rng,
     * opengl.py:124-140; Room._gen_static_data :295-297): per slot (0 wall, 1 floor, 2 ceiling —
     * the reference's draw order of rng.integers) the number of variants, their texture ids and
     * TEX_DENSITY / size (u, v).  n = 0 disables (geometry stays the shared set). */
    int32_t tex_nvar[3];
    int32_t tex_var_id[3][9];
    double tex_var_scale[3][9][2];
    double room_wall_height;    /* Room.wall_height of the generated room (2.74) */
    int32_t room_no_ceiling;    /* Room(no_ceiling=True) */
    int32_t rng_mode;           /* MW_RNG_* stream of the device generators */
} mw_config;

#define MW_POLY_ENTITY 0x100     /* a quad of a static ImageFrame / TextFrame: not drawn by mw_visible_ents            */
#define MW_POLY_XF     0x200     /* drawn under its own model transform: glTranslatef(xf[0..2]), glRotatef(xf[3], 0, 1, 0) */
#define MW_POLY_QUAD   0x400     /* issued inside glBegin(GL_QUADS) (walls, frames); otherwise GL_POLYGON (floor, ceiling) */

/* One static polygon exactly as it is fed to GL inside display list 1: a room polygon of Room._render
 * (miniworld.py:401-434, colour 1,1,1; floor and ceiling are GL_POLYGONs, walls GL_QUADS — the driver splits the two
 * kinds into different triangle pairs) or a quad of a static ImageFrame / TextFrame (entity.py:193-259, 303-383:
 * textured front in 1,1,1, border in 0,0,0) in the frame's OBJECT space with the arguments of the glTranslatef /
 * glRotatef in front of it: the engine composes the modelview like the GL matrix stack does. */
typedef struct {
    float v[4][3];              /* glVertex3f   */
    float uv[4][2];             /* glTexCoord2f */
    float n[3];                 /* glNormal3f   */
    int32_t nv;                 /* 3 or 4, | MW_POLY_* flags */
    int32_t tex;                /* texture id from mw_upload_texture, -1 = untextured */
    float rgb[3];               /* glColor3f    */
    float xf[4];                /* MW_POLY_XF: translation x, y, z and rotation angle in degrees about +y (entity.py:205-207) */
} mw_poly;

/* Host view of the world state of `count` consecutive envs; any pointer may be NULL
 * (= leave / do not fetch).  Mirrors the Python attributes the reference keeps:
 * agent.pos/dir/cam_* (entity.py:455-515), env.sky_color/light_* (miniworld.py:576-578),
 * entities[*].pos/dir/size/color_vec/scale/radius/height (entity.py), step_count, carrying. */
typedef struct {
    double *agent_pos;          /* [count][3]                                        */
    double *agent_dir;          /* [count]                                           */
    double *cam;                /* [count][4] cam_height, cam_fwd_disp, cam_pitch(deg), cam_fov_y(deg) */
    double *light;              /* [count][12] sky_color, light_pos, light_color, light_ambient */
    int32_t *carrying;          /* [count] entity slot or -1                         */
    int32_t *step_count;        /* [count]                                           */
    int32_t *num_picked_up;     /* [count]                                           */
    int32_t *ent_kind;          /* [count][max_ents] MW_ENT_* (NONE = empty / removed) */
    int32_t *ent_mesh;          /* [count][max_ents] mesh id                         */
    int32_t *ent_static;        /* [count][max_ents]                                 */
    double *ent_pos;            /* [count][max_ents][3]                              */
    double *ent_dir;            /* [count][max_ents]                                 */
    double *ent_geom;           /* [count][max_ents][9] size xyz, color rgb, scale, radius, height */
    double *extent;             /* [count][4] env.min_x, max_x, min_z, max_z (miniworld.py:588-591); top view only */
} mw_state_view;

/* ---- placement programs (MW_GEN_PROGRAM) --------------------------------------------------------------------
 * The env families beyond the four BASELINE configs have a FIXED floorplan; their _gen_world only draws a few
 * numbers and places entities (fourrooms.py:46-73, tmaze.py:54-81, ymaze.py:56-108, wallgap.py:48-77, threerooms.py:47-73,
 * putnext.py:45-65, roomobjects.py:44-80, sidewalk.py:51-91, sign.py:101-150).  The host compiles that method into
 * the table below; the device generator executes it on the env's random stream (MW_RNG_PCG64: numpy's own, so env i
 * is the reference's reset(seed + i)), for mw_reset and for the same-step auto-reset:
 *   1. the entity table is initialised from the template (ent_*: what the constructors give before placement);
 *   2. the ops run in order; the first placement op also runs Room._gen_static_data for every room (miniworld.py:856-857):
 *      with domain_rand three texture-variant draws per room, wall / floor / ceiling (opengl.py:134-138), after which
 *      the room polygons of the template are re-emitted into the env's own geometry set with the variants' texture ids
 *      and texture coordinates (metres * TEX_DENSITY / size, miniworld.py:82-119);
 *   3. the per-episode parameters, Box.randomize for every box in slot order, Agent.randomize (miniworld.py:576-585). */
#define MW_PROG_MAX_ROOMS 16
#define MW_PROG_MAX_TEX 8
#define MW_PROG_MAX_OPS 48
#define MW_PROG_MAX_ENTS 64

enum {
    MW_OP_COIN = 1,         /* reg = np_random.integers(0, n)              n in `slot`                          */
    MW_OP_DRAW_DIR = 2,     /* dir_reg = np_random.uniform(-dir, dir)      (an argument evaluated before place_entity) */
    MW_OP_PLACE = 3,        /* place_entity(ent, room=..., min_x=... ) by rejection sampling (miniworld.py:839-909)  */
    MW_OP_FIXED = 4,        /* place_entity(ent, pos=(lx, a, lz), dir=...)                                       */
    MW_OP_BOX_SIZE = 5,     /* Box(size=np_random.uniform(a, b)): size, radius, height of box `slot`             */
    MW_OP_COLOR = 6,        /* colour index = np_random.choice(6) for `slot`: room = 0 box (colour vector),
                             * 1 / 2 ball / key (mesh id = flags + index)                                        */
    MW_OP_APPEND = 7        /* self.entities.append(ent): in the list from here on (no draw, no static data)     */
};

typedef struct {
    int32_t nverts;             /* 3 or 4 outline corners, counter-clockwise seen from above (miniworld.py:127-176) */
    int32_t wall_tex, floor_tex, ceil_tex;      /* indices into mw_gen_program.tex_* (texture NAMES)             */
    double ox[4], oz[4];        /* Room.outline                                                                   */
    double nx[4], nz[4];        /* Room.edge_norms (for point_inside, miniworld.py:272-284)                       */
    double min_x, max_x, min_z, max_z;
    double cdf;                 /* cumulative room probability: np_random.choice(len(rooms), p=room_probs) picks
                                 * searchsorted(cdf, u, side="right") (miniworld.py:873-875)                      */
} mw_prog_room;

typedef struct {
    int32_t op;                 /* MW_OP_*                                                                         */
    int32_t slot;               /* entity slot; -1 = the agent                                                     */
    int32_t room;               /* PLACE: room index, -1 = choice over all rooms                                   */
    int32_t cond;               /* run only if the coin register == cond (-1: always)                              */
    int32_t dir_mode;           /* 0: uniform(-pi, pi) drawn after the position; 1: `dir`; 2: the DRAW_DIR register */
    int32_t flags;              /* PLACE: bit 0..3 = min_x, max_x, min_z, max_z given (lx, hx, lz, hz)             */
    double lx, hx, lz, hz;
    double dir;
    double a, b;
} mw_prog_op;

typedef struct {
    int32_t n_rooms, n_tex, n_ops, n_ents;
    mw_prog_room rooms[MW_PROG_MAX_ROOMS];
    int32_t tex_nvar[MW_PROG_MAX_TEX];          /* variants of each texture name (Texture.get, opengl.py:124-140) */
    int32_t tex_var_id[MW_PROG_MAX_TEX][9];     /* their texture ids (mw_upload_texture)                           */
    double tex_var_scale[MW_PROG_MAX_TEX][9][2];/* TEX_DENSITY / (width, height)                                   */
    mw_prog_op ops[MW_PROG_MAX_OPS];
    int32_t ent_kind[MW_PROG_MAX_ENTS], ent_mesh[MW_PROG_MAX_ENTS], ent_static[MW_PROG_MAX_ENTS];
    double ent_pos[MW_PROG_MAX_ENTS][3], ent_dir[MW_PROG_MAX_ENTS], ent_geom[MW_PROG_MAX_ENTS][9];
    double colors[6][3];        /* COLORS of the six sorted colour names (entity.py:30-43), for MW_OP_COLOR         */
    double extent[4];           /* env.min_x, max_x, min_z, max_z                                                  */
    double street[4];           /* MW_TASK_SIDEWALK: min_x, max_x, min_z, max_z of the forbidden room              */
    int32_t sign_n, pad;        /* MW_TASK_SIGN: objects in the order sign.py:160-169 visits them                  */
    int32_t sign_slot[8];
    double sign_reward[8];
} mw_gen_program;

/* Installs the placement program of an engine created with MW_GEN_PROGRAM.  The template geometry (what
 * mw_set_geometry would receive for domain_rand = 0) comes with, per polygon, the room it belongs to (-1: not a room
 * polygon, copied as it is), its surface (0 wall, 1 floor, 2 ceiling) and the metre coordinates its texture
 * coordinates are computed from (poly_m[p][k] = the two factors of vertex k), so that a texture-variant draw can
 * re-emit it.  With shared_geometry = 1 (no texture randomisation) the template is installed as the shared set. */
int mw_set_gen_program(mw_engine *e, const mw_gen_program *prog, const mw_poly *polys, const int32_t *poly_room,
                       const int32_t *poly_surf, const double *poly_m /* [n_polys][4][2] */, int32_t n_polys,
                       const double *segs, int32_t n_segs);

/* ---- lifetime --------------------------------------------------------------- */
/* replaces MiniWorldEnv.__init__'s GL setup (shadow window, FrameBuffer) miniworld.py:504-518 */
int mw_create(const mw_config *cfg, mw_engine **out);
void mw_destroy(mw_engine *e);
/* last error message of `e` (or of the failed mw_create when e == NULL) */
const char *mw_last_error(const mw_engine *e);

/* ---- assets ----------------------------------------------------------------- */
/* replaces Texture.load (opengl.py:148-184): RGB8, rows bottom-up; builds the mip pyramid */
int mw_upload_texture(mw_engine *e, int32_t tex_id, const uint8_t *rgb_bottom_up, int32_t w, int32_t h);
/* replaces ObjMesh's vertex lists (objmesh.py:139-207): per-face-vertex arrays [ntris][3][k] (pos, nrm, rgb:
 * k = 3; uv: k = 2); tex_id = the chunk's map_Kd texture (objmesh.py:209-216, 280-292) or -1 */
int mw_upload_mesh(mw_engine *e, int32_t mesh_id, const float *pos, const float *nrm, const float *uv,
                   const float *rgb, int32_t ntris, int32_t tex_id);

/* ---- world ------------------------------------------------------------------ */
/* replaces Room._gen_static_data + _render_static's display list (miniworld.py:286-399,
 * 1019-1062) and env.wall_segs (:998-999).  env = -1 for the shared set.
 * segs: [n_segs][2][2] (x,z of both endpoints). */
int mw_set_geometry(mw_engine *e, int32_t env, const mw_poly *polys, int32_t n_polys,
                    const double *segs, int32_t n_segs);
/* state injection / inspection (synchronous) */
/* reads one geometry set back (polys: max_polys entries, segs: max_segs*4 doubles) */
int mw_get_geometry(mw_engine *e, int32_t env, mw_poly *polys, int32_t *n_polys, double *segs, int32_t *n_segs);
/* (clears a pending next-step auto-reset of the envs it writes)
 * Domain: |agent_dir| < 1e6 radians — the agent's heading feeds the f64 sin / cos of the dynamics and the camera
 * (mw_math.h sincos_det, within 1 ulp of libm there and no further).  An entity's dir may be any finite angle: it only
 * feeds the float rotation of glRotatef (mw_glmath.h sincosf_glibc, glibc's bits for every float). */
int mw_set_state(mw_engine *e, int32_t first_env, int32_t count, const mw_state_view *host);
/* Test hook: host double[num_envs][3] = forward_step, forward_drift, turn_step to use in
 * the next steps instead of the defaults / device RNG draws (miniworld.py:678-680);
 * NULL switches the override off. */
int mw_set_step_params(mw_engine *e, const double *host_params);
int mw_get_state(mw_engine *e, int32_t first_env, int32_t count, mw_state_view *host);
/* State views on the device: what research code around the reference reads and writes as plain Python attributes — env.agent.pos and
 * env.agent.dir, env.agent.carrying, env.entities[k].pos, env.step_count (entity.py:455-515, miniworld.py:576-578; the attributes
 * mw_state_view lists) — for an asymmetric critic, a visitation count, a scripted expert, the cell key of an archive, a start-state
 * curriculum, without the synchronisation, the per-component copies and the host transposition of mw_get_state / mw_set_state.  Both
 * calls take the same struct: it stays in HOST memory, its pointers are DEVICE pointers (torch tensors), any may be NULL (= leave / do
 * not fetch).  One kernel launch each, asynchronous on `stream`, no host value read, no synchronisation.
 *
 * mw_get_state_device: rows of envs first_env .. first_env + count - 1, laid out exactly as mw_get_state lays them out on the host
 * ([count][3], [count], [count][max_ents][9], ...), bit for bit what mw_get_state would return at that point of the stream: ent_kind
 * MW_ENT_NONE for a removed slot, a picked-up object still listed until the frame's tail removed it, the new episode's state for an env
 * a same-step auto-reset just restarted, the terminal state under MW_AUTORESET_NEXT_STEP.  It reads live state only and changes
 * nothing in the engine.  count == 0 is MW_OK and launches nothing.  MW_E_INVALID before anything is launched: a null engine or view,
 * a range outside 0 .. num_envs, a view whose pointers are all NULL. */
int mw_get_state_device(mw_engine *e, int32_t first_env, int32_t count, const mw_state_view *d_view, void *stream);
/* mw_set_state_where: rows are [N][...] over ALL num_envs envs, d_mask is uint8[N] on the device.  For every env i with d_mask[i] != 0,
 * row i of each non-null field is written into the engine's state: mid-episode injection with mw_set_state's meaning (and its domain of
 * agent_dir) — no consistency is made between fields.  Row i of any field is not read where d_mask[i] == 0: garbage or NaN under a zero
 * mask byte is never an error.  The grid covers all N envs whatever the mask holds.  `extent` may be written; it is a top-view value.
 * What each written env is owed, on the device (the pattern of mw_snapshot_load_where): its pending next-step auto-reset is dropped
 * and, as by mw_set_state, the rebuild of its frame stack that reset would have caused (the stacks themselves stay); its frame-clean
 * byte is cleared; its frame-cache epoch advances, so none of its cached frames can match again.  Nothing is owed to any other env:
 * their cached frames stay valid, where mw_set_state drops every env's.  On the host the held frame of frame reuse is dropped (the
 * caller's buffers no longer show the masked envs): draw next (mw_render), or step — the step draws every env it cannot serve from the
 * frame cache.
 * Validation on the device: a masked env whose `carrying` lies outside -1 .. max_ents - 1 or one of whose `ent_kind` lies outside
 * MW_ENT_NONE .. MW_ENT_FRAME is skipped whole — it writes nothing — and sets a status bit that the next mw_check reports as
 * MW_E_INVALID, once, ahead of whatever else the status word holds (the check after it reports that); the other envs are written as usual.  MW_E_INVALID before anything is launched: a null engine, mask or view, a
 * view whose pointers are all NULL. */
int mw_set_state_where(mw_engine *e, const uint8_t *d_mask, const mw_state_view *d_view, void *stream);
/* device-side MiniWorldEnv.reset (miniworld.py:544-604) for the configured generator.
 * mask: host uint8[num_envs] or NULL (= all); seeds: host uint64[num_envs] or NULL.
 * With MW_GEN_NONE (host-generated worlds) only the re-seeding happens: seeds[i] (masked) re-seeds env i's device
 * stream, which serves the per-step domain-randomisation draws (miniworld.py:677-680); seeds == NULL is an error.
 * A pending next-step auto-reset of a reset env is dropped (the env's next step is an ordinary one), and so is the mark that an
 * entity has just left its list (mw_get_frame_clean): nothing of the old episode's last pickup reaches the new world's first step.
 * With a frame stack (mw_set_frame_stack) the envs whose world it writes are marked: mw_stack_refresh or their next push rebuilds
 * their stacks (a MW_GEN_NONE engine's reset writes no world and marks nothing). */
int mw_reset(mw_engine *e, const uint8_t *mask, const uint64_t *seeds, void *stream);
/* The device twin of mw_reset(mask, seeds): MiniWorldEnv.reset(seed=...) (miniworld.py:544-604) of the masked envs with both arrays
 * ON THE DEVICE — what a loop that restarts finished envs from chosen seeds (Procgen's start_level / num_levels, seed-based level
 * replay, evaluation on held-out seeds) calls behind a step without learning on the host which envs finished.
 *   d_mask   uint8[N], device
 *   d_seeds  uint64[N], device; d_seeds[i] is not read where d_mask[i] == 0
 * Asynchronous on `stream`: no host synchronisation, no host value read, the stream array never leaves the device.  For every masked
 * env: its stream is re-seeded on the device with the arithmetic the host seeds with (numpy's SeedSequence + PCG64 under MW_RNG_PCG64;
 * key = seed, counter 0 under MW_RNG_PHILOX), the live world is generated directly from it (a pre-generated next world goes stale and
 * is marked for regeneration), a pending next-step auto-reset is dropped, the env's frame-cache epoch advances and, with a frame stack,
 * its stack flag is marked as after mw_reset.  Nothing of any other env is written: the call leaves the other envs' cached frames
 * alone.  It does drop the held frame of frame reuse (the caller's buffers no longer show the masked envs): draw next (mw_render).
 * MW_GEN_NONE: the masked envs are re-seeded only, as by mw_reset.
 * MW_E_INVALID, before anything is launched: a null engine, mask or seeds; MW_GEN_PROGRAM without a program. */
int mw_reset_where(mw_engine *e, const uint8_t *d_mask, const uint64_t *d_seeds, void *stream);

/* ---- the hot path ------------------------------------------------------------ */
/* MiniWorldEnv.step (miniworld.py:670-730) + env rule + render_obs (:1177-1221) for all envs.
 *   d_actions int32[N]            MiniWorldEnv.Actions (:451-468)
 *   d_obs     uint8[N][H][W][3]   FrameBuffer.resolve() layout, row 0 = top (opengl.py:339-398)
 *   d_depth   float[N][H][W][1]   FrameBuffer.get_depth_map(0.04, 100) (opengl.py:400-435); NULL = skip
 *   d_reward  float[N], d_term uint8[N], d_trunc uint8[N]
 * All device pointers; asynchronous on `stream`.  Auto-reset of finished envs: mw_config.autoreset (MW_AUTORESET_*).  With
 * MW_AUTORESET_NEXT_STEP, mw_render / mw_render_top / mw_get_state / mw_get_info between the step that ends an episode and the next
 * step see the terminal state. */
int mw_step(mw_engine *e, const int32_t *d_actions, uint8_t *d_obs, float *d_depth,
            float *d_reward, uint8_t *d_term, uint8_t *d_trunc, void *stream);
/* Action repeat (gymnasium's frame skip, DMLab's action repeat): up to `repeat` consecutive MiniWorldEnv.step(action) per env with
 * the same action, in ONE step-kernel launch, and one frame at the end.  Arguments as mw_step's, and
 *   repeat    1 .. MW_MAX_REPEAT; anything else is MW_E_INVALID: nothing is launched, no state is touched
 *   d_nsteps  int32[N] or NULL: the sub-steps the env executed in this call
 * Per env and call:
 *   - sub-steps 1, 2, ... are each exactly mw_step's step: physics, the env rule, step_count + 1 — max_episode_steps counts
 *     sub-steps, as a frame-skip wrapper around the reference env would; with domain randomisation every executed sub-step takes its
 *     three per-step draws from the env's stream (miniworld.py:677-680), with mw_set_step_params the override values.
 *   - the env stops after the first sub-step that sets term | trunc; d_term / d_trunc are that last executed sub-step's flags;
 *     d_reward is the sum of the executed sub-steps' rewards, taken in double, in order, rounded to float once.
 *   - between two sub-steps the step kernel applies what the frame's tail applies after a rendered step: a picked-up object leaves
 *     the entity list (pickupobjects.py:86-88), MW_TASK_COLLECT's consumed kit respawns with its draws from the env's stream (the
 *     sub-step's draws, the respawn's, then the next sub-step's).  The last executed sub-step's removal is applied behind the frame
 *     as after mw_step: the object is drawn one last time.
 *   - auto-reset is applied once, after the last executed sub-step.  MW_AUTORESET_SAME_STEP: an env that finished installs its next
 *     world, the frame is the new episode's first and the remaining repeats are dropped — an env never steps in two episodes within
 *     one call.  MW_AUTORESET_NEXT_STEP: the call that ends an episode returns the terminal frame; the env's next call executes 0
 *     sub-steps whatever `repeat` is — it installs the next world, reward 0, no flags, d_nsteps 0.  MW_AUTORESET_OFF or
 *     MW_GEN_NONE: the env stops at its terminal state and the frame shows it.  With final buffers (mw_set_final_obs) the call
 *     takes mw_step's two passes.
 *   - mw_get_info, mw_get_final_info and mw_get_reset_pending behave as after an mw_step that ended with the call's last sub-step;
 *     the frame-clean byte (mw_get_frame_clean) is 1 iff the env executed at least one sub-step and every executed sub-step left
 *     its state as it was; frame reuse treats the call as a plain step of the whole batch.
 * repeat = 1 returns what mw_step returns, bit for bit (through the repeat kernels; mw_step keeps the plain ones). */
#define MW_MAX_REPEAT 256       /* keeps one launch bounded */
int mw_step_repeat(mw_engine *e, const int32_t *d_actions, int32_t repeat, uint8_t *d_obs, float *d_depth,
                   float *d_reward, uint8_t *d_term, uint8_t *d_trunc, int32_t *d_nsteps, void *stream);
/* Open-loop rollouts (the inner loop of CEM, MPPI, random shooting, a tree search's rollout phase): up to `horizon` consecutive
 * MiniWorldEnv.step(plan[k]) per env in ONE step-kernel launch, and one frame at the end or none at all — the reference's
 * step() / render_obs() split (miniworld.py:670-730 / :1177-1221), T times step() without the T render_obs().  Arguments as
 * mw_step_repeat's, and
 *   d_plans        int32[horizon][N], sub-step-major: sub-step k of env i takes d_plans[k][i]
 *   horizon        1 .. MW_MAX_PLAN; anything else is MW_E_INVALID: nothing is launched, no state is touched
 *   d_step_reward  float[horizon][N] or NULL: the reward a single mw_step would have returned for sub-step k; 0 for every sub-step
 *                  the env did not execute (what a planner discounts from)
 *   d_obs          NULL: a FRAMELESS call (d_depth must be NULL too, else MW_E_INVALID)
 * Per env and call: `for k in range(horizon): step(d_plans[k][env]); if done: break`, then the auto-reset of the engine's mode — every
 * clause of mw_step_repeat's contract above with "the action" read as "row k's action": the env stops at the first sub-step that sets
 * term | trunc, flags are that sub-step's, d_reward is the executed sub-steps' sum (in double, in order, rounded once), d_nsteps
 * their count; max_episode_steps counts sub-steps and every executed one takes its three domain-randomisation draws; the auto-reset
 * runs once, behind the last executed sub-step; a next-step env that enters with reset_pending executes 0 sub-steps and installs its
 * world; the env's stream is consumed as sub-step 1's draws, what follows it, sub-step 2's draws, ..., then the reset's.
 * A DRAWN call (d_obs != NULL) is mw_step_repeat behind the step kernel: one frame, the frame's tail, frame reuse and the frame cache,
 * the two passes with final buffers, one stack push.  A plan whose rows are all equal returns, bit for bit, what
 * mw_step_repeat(repeat = horizon) returns, and horizon = 1 what mw_step returns.
 * A FRAMELESS call launches the step kernel (in the engine's own auto-reset mode, final buffers or not) and nothing that draws: no
 * geometry, raster or respawn kernel, no push, no final-buffer pass.  The step kernel applies, behind the last executed sub-step, what
 * the frame's tail of a drawn call would have: a picked-up object leaves the list (pickupobjects.py:86-88), MW_TASK_COLLECT's consumed
 * kit respawns with its draws from the env's stream (collecthealth.py:79-98) — also on a next-step terminal sub-step, where the
 * reference's loop draws the respawn before reset(); not when that sub-step installed a world (same-step drops it, as mw_step does).
 * Afterwards the state, the stream, mw_get_info / mw_get_final_info / mw_get_reset_pending are those of `horizon` mw_steps with a host
 * that reads no frame, and mw_render draws that state.  d_obs, d_depth, the final buffers and the stack's ring keep what they held:
 * mw_get_frame_clean reports 0 for every env, the frame that frame reuse holds is dropped (the next drawn call draws every env),
 * the frame cache is neither read nor filled and stays valid.  mw_kernel_time_ms does not sample frameless calls.
 * Frame stack: a frameless call pushes nothing and the ring position stays.  The first push after any number of frameless calls
 * rebuilds the stack of exactly those envs that began a new episode since their last push; every other env's window gains that
 * call's frame as usual. */
#define MW_MAX_PLAN MW_MAX_REPEAT
int mw_step_plan(mw_engine *e, const int32_t *d_plans /* [horizon][N] */, int32_t horizon,
                 uint8_t *d_obs, float *d_depth, float *d_reward, float *d_step_reward /* [horizon][N] or NULL */,
                 uint8_t *d_term, uint8_t *d_trunc, int32_t *d_nsteps, void *stream);
/* Rollout traces: mw_step_plan, and where the agent was after each of its sub-steps — what a planner turns into a dense cost on the
 * device (the distance to a goal, a visitation count, an archive's cell key) where the rewards are sparse.  The fields are those of
 * env.agent and env.entities that step() itself writes (miniworld.py:670-730; the carried entity follows the agent, entity.py:455-515)
 * and the frame's tail never touches.  A host struct of DEVICE pointers; any may be NULL, not all:
 *   agent_pos  double[horizon][N][3]  env.agent.pos as step() k leaves it
 *   agent_dir  double[horizon][N]     env.agent.dir
 *   carrying   int32[horizon][N]      the carried slot or -1, as the step stores it: a MW_TASK_PICKUP object that leaves the list reads -1
 *   ent_pos    double[horizon][N][3]  the position of ONE slot, ent_slot (0 .. max_ents - 1) — the goal box, or the box being carried.
 *                                     The slot's kind is not consulted: a removed slot keeps its last position.
 * Row k of env i is the state the env is in when its sub-step k (0-based) has run its physics and its rule, before any auto-reset: each
 * row has mw_state_view's row layout and holds, bit for bit, what mw_get_state_device returns for that field behind a single mw_step
 * of a MW_AUTORESET_OFF engine in the same state.  The terminal sub-step's row is the terminal state in every auto-reset mode (the world a
 * same-step engine installs on it never shows).  Rows k >= d_nsteps[i] repeat row d_nsteps[i] - 1 — the env stays where it ended, a
 * cost summed over the horizon needs no mask —, and all rows of an env that executed 0 sub-steps (next-step, entered with
 * reset_pending) hold the state it entered the call with.  Exactly `horizon` rows of N columns are written, by the step kernel itself
 * (the trace kernels, mode 3 of the step kernel's table in mw_kernels.h: the plan kernels with the stores added; mw_step_plan keeps its own).
 * Everything else is mw_step_plan's contract, clause for clause — drawn or frameless, final buffers, reset seeds, the stack, frame
 * reuse and the frame cache: state, stream, frames, rewards, flags, d_nsteps and d_step_reward are bit for bit what mw_step_plan returns.
 * MW_E_INVALID, nothing launched and nothing touched: `trace` NULL or without a field; ent_pos with ent_slot out of range; ent_pos
 * on a MW_TASK_COLLECT engine (a kit's respawn belongs to the frame's tail, so where it is after sub-step k would depend on whether a
 * frame follows); whatever mw_step_plan refuses. */
typedef struct {            /* host struct, DEVICE pointers; any may be NULL, not all */
    double  *agent_pos;     /* [horizon][N][3] */
    double  *agent_dir;     /* [horizon][N]    */
    int32_t *carrying;      /* [horizon][N]    */
    double  *ent_pos;       /* [horizon][N][3], slot ent_slot */
    int32_t  ent_slot;
} mw_plan_trace;
int mw_step_plan_trace(mw_engine *e, const int32_t *d_plans, int32_t horizon, uint8_t *d_obs, float *d_depth,
                       float *d_reward, float *d_step_reward, uint8_t *d_term, uint8_t *d_trunc, int32_t *d_nsteps,
                       const mw_plan_trace *trace, void *stream);
/* Final observations of a MW_AUTORESET_SAME_STEP engine (Gymnasium's info["final_obs"] of a same-step vector env, SB3's
 * info["terminal_observation"]): d_final_obs and d_final_depth are device buffers shaped like mw_step's d_obs / d_depth (N rows in
 * the layout of mw_set_obs_layout at the time of the step).  With d_final_obs non-null, every later mw_step writes the TERMINAL
 * frame of each env whose episode ended in that step (term | trunc) into that env's row of d_final_obs — and its depth into
 * d_final_depth when both the step's d_depth and d_final_depth are non-null.  The rows of the other envs are not written.
 * Everything else the step returns is what same-step returns without it: d_obs (the next episode's first frame), reward, flags,
 * mw_get_state, mw_get_info, mw_get_final_info; mw_get_reset_pending stays all zeros.  Still asynchronous and without host
 * synchronisation: the step draws every env, then the finished ones once more (their new worlds).  NULL turns it off again.
 * MW_E_INVALID on MW_AUTORESET_OFF / MW_AUTORESET_NEXT_STEP engines and on MW_GEN_NONE engines (nothing is auto-reset there: the
 * frame mw_step returns is the terminal one). */
int mw_set_final_obs(mw_engine *e, uint8_t *d_final_obs, float *d_final_depth);
/* Seeded same-step auto-reset: d_next_seed is the caller's uint64[N] on the device (NULL turns it off again).  With it set, an env
 * whose episode ends in a step starts, in that step, the episode MiniWorldEnv.reset(seed=d_next_seed[i]) starts (miniworld.py:544-604)
 * instead of continuing on its own stream as the reference's benchmark loop does (scripts/benchmark.py:36-37): its stream is re-seeded
 * on the device and its world generated from it.  d_next_seed[i] is read only for an env that finishes in a call, and at that call,
 * on the call's stream: the caller may rewrite the array between calls on the same stream (a level sampler writes its choices there).
 * Every drawn mw_step, mw_step_repeat and mw_step_plan then takes the two passes of a step with final buffers, whether or not final
 * buffers are set: the step as the next-step mode's terminal step and the frame of every env; the finished envs' rows into the final
 * buffers where set (the two compose); the listed envs seeded and generated; the frame of those envs alone.  What the call returns is
 * the same-step contract: the observation returned with term | trunc is the first frame of the episode of d_next_seed[i], reward and
 * flags are the finished episode's, mw_get_final_info reports it, mw_get_reset_pending stays zeros, one stack push rebuilds the
 * finished envs' stacks.  The step's own draws (domain randomisation, MW_TASK_COLLECT) on the terminal step come from the old stream.
 * A pre-generated next world is never used while seeds are set; it is regenerated from the new stream like any consumed one.  Frame
 * reuse and the frame cache serve the first pass as they serve a plain step.  After NULL the envs continue as plain same-step
 * auto-reset on their current streams.
 * MW_E_INVALID on MW_AUTORESET_OFF / MW_AUTORESET_NEXT_STEP engines and on MW_GEN_NONE engines (mw_set_final_obs's rule).  While seeds
 * are set a FRAMELESS mw_step_plan (d_obs == NULL) is MW_E_INVALID and touches nothing: the step kernel cannot seed. */
int mw_set_reset_seeds(mw_engine *e, const uint64_t *d_next_seed /* [N], device; NULL = off */);
/* Frame stacking on the device (Gymnasium's FrameStackObservation, SB3's VecFrameStack, EnvPool's stack_num around the reference env):
 * the engine keeps the last `depth` frames each env RETURNED — its rows of d_obs, in the layout of mw_set_obs_layout; depth maps are
 * not stacked — oldest first, in the caller's ring.
 *   depth         2 .. MW_MAX_STACK; 0 (or d_ring == NULL) turns the stack off
 *   pad           what fills a new episode's stack: MW_STACK_PAD_RESET depth copies of its first frame (Gymnasium's
 *                 padding_type="reset"), MW_STACK_PAD_ZERO depth - 1 all-zero frames, then the frame (SB3's VecFrameStack)
 *   d_ring        [N][2 * depth - 1][frame bytes].  Push number j of the engine (0, 1, ...) writes an env's frame to slot
 *                 (j mod depth) + depth - 1 and, when j mod depth >= 1, to slot (j mod depth) - 1 too; after it the ordered window of
 *                 every env is the `depth` consecutive slots from slot j mod depth on (mw_stack_window) — nothing is ever shifted
 *   d_final_stack [N][depth][frame bytes] or NULL; used by the steps of an engine with final buffers (mw_set_final_obs), and
 *                 MW_E_INVALID where mw_set_final_obs is (not MW_AUTORESET_SAME_STEP, or MW_GEN_NONE)
 * A depth outside 2 .. MW_MAX_STACK or an unknown pad is MW_E_INVALID and changes nothing.  Setting a stack marks every env "never
 * pushed", restarts j at 0 and remembers the layout: a step or refresh under another layout is MW_E_INVALID before anything is
 * launched (mw_render / mw_render_top under another layout push nothing and stay legal).
 * One push ends every mw_step and every mw_step_repeat (one per call: the stack holds the frames the agent saw), asynchronous on the
 * call's stream behind its last raster kernel; everything else the call returns is bit for bit what it returns without a stack,
 * frame reuse included (the push reads the rows of clean envs where they lie).  Per env and push:
 *   - an ordinary frame: the window drops its oldest frame and gains the call's; afterwards its newest frame is the env's row of d_obs.
 *   - the first frame of an episode: the env's whole stack is rebuilt from that frame and the pad.  That is: the call installed a
 *     world for the env through auto-reset (same-step: the call set term | trunc and a generator is configured; next-step: the env
 *     entered the call with reset_pending); or mw_reset wrote the env's world since its last push; or the env was never pushed.  With
 *     MW_AUTORESET_OFF or MW_GEN_NONE a finished env keeps stacking its terminal state's frames until the host resets it.
 *   - mw_set_state is mid-episode injection and leaves stacks alone; as it clears a pending next-step reset, it also cancels the
 *     rebuild that reset would have caused.
 *   - final stacks (final buffers and d_final_stack both set): for every env whose episode ended in the call, its row of
 *     d_final_stack = its depth - 1 newest frames from before this push (zeros where the zero pad still shows; the pad alone for an
 *     env without a valid stack: reset or never pushed, and not refreshed), then its terminal frame, the row mw_set_final_obs
 *     writes.  The rows of the other envs are not written. */
#define MW_MAX_STACK 16
enum { MW_STACK_PAD_RESET = 0, MW_STACK_PAD_ZERO = 1 };
int mw_set_frame_stack(mw_engine *e, int32_t depth, int32_t pad, uint8_t *d_ring, uint8_t *d_final_stack /* [N][depth][frame] or NULL */);
/* The reset path of a frame stack (FrameStackObservation.reset, VecFrameStack.reset): rebuilds, from their rows of d_obs, the stacks of
 * exactly those envs that mw_reset wrote since their last push or that were never pushed; every other env and the ring position stay
 * as they are.  The host sequence is mw_reset(mask), mw_render(d_obs), mw_stack_refresh(d_obs); an env reset without a refresh is
 * rebuilt by its next push instead.  Asynchronous on `stream`; MW_E_INVALID without a stack or under another layout than the stack's. */
int mw_stack_refresh(mw_engine *e, const uint8_t *d_obs, void *stream);
/* Where the ordered window lies (the view FrameStackObservation / VecFrameStack hand out as the observation): *first_slot = the slot
 * of every env's oldest frame — stack[env][k] = d_ring[env][*first_slot + k], k = 0 .. depth - 1 —, *pushes = the pushes since
 * mw_set_frame_stack.  Host values, no synchronisation; either pointer may be NULL; MW_E_INVALID without a stack. */
int mw_stack_window(const mw_engine *e, int32_t *first_slot, int64_t *pushes);   /* host values, no sync */
/* Layout of the d_obs buffer written by mw_step / mw_render / mw_render_top — the reference's
 * observation wrappers (wrappers.py) folded into the raster kernel's store:
 *   MW_OBS_HWC_U8   uint8 [N][H][W][3]   the env's own observation (default)
 *   MW_OBS_CWH_U8   uint8 [N][3][W][H]   PyTorchObsWrapper.observation: transpose(2, 1, 0)   (wrappers.py:11-25)
 *   MW_OBS_GREY_F64 double[N][H][W][1]   GreyscaleWrapper.observation: 0.30 R + 0.59 G + 0.11 B evaluated as
 *                                        numpy does, in float64, left to right             (wrappers.py:28-46) */
enum { MW_OBS_HWC_U8 = 0, MW_OBS_CWH_U8 = 1, MW_OBS_GREY_F64 = 2 };
int mw_set_obs_layout(mw_engine *e, int32_t layout);

/* Test hook, host only (no device, no engine): the first n draws of the MW_RNG_PCG64 stream for `seed`, with the very
 * functions the device generators inline.  bounds[i] == 0 (or bounds == NULL): a double in [0, 1), i.e.
 * Generator(PCG64(SeedSequence(seed))).random(); bounds[i] = k > 0: an integer in [0, k), i.e. Generator.integers(0, k)
 * / Generator.choice(k), returned as a double. */
int mw_pcg64_draws(uint64_t seed, int32_t n, const int32_t *bounds, double *out);

/* Test hooks, GPU only, no engine (tests/test_gpu_numerics.py): the kernels' 3-instruction reciprocal / quotient
 * (hardware estimate + fused Newton / Markstein steps, mw_raster_common.h) against the IEEE division the oracle
 * performs — mw_selftest_rcp over all 2^32 floats (bad_per_exp[512]: mismatches per sign|exponent, examples[64],
 * *n = their total), mw_selftest_div over 2^32 pseudo-random pairs of its domain. */
int mw_selftest_rcp(unsigned long long *bad_per_exp, uint32_t *examples, uint32_t *n);
int mw_selftest_div(unsigned long long *n_bad, uint32_t *examples);
/* ... and the geometry kernel's visiting-order sort (mw_geom.hip: up to 512 keys per block, bitonic, in registers) on the
 * caller's keys: keys[blocks][512], n[blocks], order[blocks][513] (order[b][1 + k] = low 16 bits of block b's k-th smallest key). */
int mw_selftest_sort(const uint32_t *keys, const int32_t *n, int32_t blocks, uint16_t *order);
/* ... and two shortcuts of the quad raster kernel (mw_rasterq.hip) for all 2^32 floats: n_bad[0] = inputs where
 * v_cvt_pk_u8_f32(x * (255 / S)) differs from FrameBuffer.resolve()'s unorm8 conversion of x * (1 / S) (S = 4, 8);
 * n_bad[1] = inputs where the lod taken from rho^2's bits differs from llvmpipe's float arithmetic (pyramids of 1 .. 12
 * levels); examples[2][32] = the first offending bit patterns of each. */
int mw_selftest_q(unsigned long long *n_bad, uint32_t *examples);
/* ... and the rotations' and headings' sin / cos: sums[512] = per binade (sign | exponent) of the input, the sum mod 2^64
 * of mwcheck::hash_sincosf(x, sin, cos) (mw_selftest.h) of mwgl::sincosf_glibc over all 2^32 floats; sums64[120] = per
 * bin of mwcheck::heading_sample, the sum of mwcheck::hash_sincos(x, sin, cos) of mw::sincos_det over inputs 0 .. n64 - 1
 * of that stream.  The host forms the same sums from libm's sinf / cosf and the oracle's mwo_sincos. */
int mw_selftest_sincosf(unsigned long long *sums, unsigned long long n64, unsigned long long *sums64);

/* render_obs / render_depth only (miniworld.py:1177-1236) */
int mw_render(mw_engine *e, uint8_t *d_obs, float *d_depth, void *stream);
/* render_top_view (miniworld.py:1088-1175): orthographic map of the whole floorplan into the same
 * kind of buffers; render_agent != 0 also draws Agent.render's marker (entity.py:518-539) */
int mw_render_top(mw_engine *e, uint8_t *d_obs, float *d_depth, int32_t render_agent, void *stream);
/* render() / render_obs(vis_fb) / render_top_view(vis_fb) (miniworld.py:1340-1362): ONE env into a frame
 * buffer of any size (1 x 1 to 4080 x 1020) with msaa = 1, 4, 8 or 16 samples (vis_fb = FrameBuffer(800, 600, 16),
 * miniworld.py:518).  view_flags: bit 0 top view, bit 1 draw the agent marker.
 *   d_out uint8[height][width][3], d_depth float[height][width] or NULL.  Not the hot path. */
int mw_render_view(mw_engine *e, int32_t env, int32_t view_flags, int32_t width, int32_t height, int32_t msaa,
                   uint8_t *d_out, float *d_depth, void *stream);
/* get_visible_ents (miniworld.py:1238-1333) for envs [first_env, first_env + count): rooms drawn depth-only
 * into the obs frame, then one GL_ANY_SAMPLES_PASSED query per entity around its 0.2 m proxy box, in
 * entity-slot (= self.entities) order with depth writes on.  d_vis uint8[count][max_ents], 1 = visible;
 * empty slots report 0.  Needs obs_width * obs_height * 32 bytes of LDS (<= 160 KiB).  Not the hot path. */
int mw_visible_ents(mw_engine *e, int32_t first_env, int32_t count, uint8_t *d_vis, void *stream);

/* ---- snapshots: save, restore and fork environments on the device ------------------------------------------------
 * The reference keeps an env's state in Python attributes and its stream in env.np_random; copy.deepcopy(env) is how a user of
 * it checkpoints or branches one env.  These three calls do that for the batched engine, on the device: a RECORD is the complete
 * state of one env, a caller-owned device buffer holds `capacity` of them, and a restored or forked env continues exactly — bit for
 * bit, random stream included — as the env the record was taken from would have.
 *   record      everything that decides the env's future and is not configuration: agent pose, cam, light, extent, carry, step,
 *               picked, health, final_health, final_goal (mw_get_final_info), the entity slabs, the random stream (all five words),
 *               the pending removal (none, a slot, or "applied"), a pending next-step reset; with per-env geometry sets
 *               (shared_geometry = 0) the env's polygons and segments; in spare mode (a pre-generated next world per env) the whole
 *               spare world and its state word — the live stream has already moved past the spare's draws.
 *   NOT in it   textures, meshes, the placement program and the shared geometry set (configuration); the mw_set_step_params
 *               override; rendered frames and the frame-stack ring; all per-frame scratch.
 *   the buffer  opaque.  It starts with a header that carries a layout key — a format number, max_ents, max_polys, max_segs,
 *               shared_geometry, task, generator, rng_mode, spares on / off, capacity — and is compatible between engines of the
 *               same configuration in one process, whatever their num_envs.  It must be 16-byte aligned.
 * d_envs and d_recs are DEVICE arrays (a planner picks on the device which state to branch from); both calls are asynchronous on
 * `stream` and one kernel launch each.  They wait, on `stream` (an event: the host does not block), for the spare-world refills the
 * Maze's steps leave running on the engine's side stream.
 * Errors.  MW_E_INVALID before anything is launched: a null engine or buffer, a misaligned buffer, count < 0, count > capacity,
 * count > num_envs on a load or on a save with d_envs == NULL, n_recs > capacity.  On the device every env and record index is
 * tested against its limit and a load compares the header's key: an offending item is skipped — it writes nothing — and sets a bit
 * of the status word that mw_check reports as MW_E_INVALID. */
/* bytes of a caller-owned device buffer that holds `capacity` records of this engine (host value, no sync; < 0 on error) */
int64_t mw_snapshot_bytes(const mw_engine *e, int32_t capacity);
/* record k (k < count <= capacity) := the complete state of env d_envs[k]; d_envs == NULL: env k, count <= num_envs.  Writes the header.
 * Changes nothing in the engine. */
int mw_snapshot_save(mw_engine *e, const int32_t *d_envs, int32_t count, uint8_t *d_snap, int32_t capacity, void *stream);
/* env d_envs[k] := record d_recs[k] of a buffer whose first n_recs records are valid.  d_envs == NULL: env k.  d_recs == NULL: record k.
 * The target envs must be distinct (caller's contract); records may repeat (that is a fork).
 * Like mw_set_state it drops the frame that frame reuse holds; for every env it writes it clears the frame-clean byte, invalidates
 * the occlusion cache of the env's geometry set and, with a frame stack, marks the env like mw_reset does: mw_stack_refresh or its next
 * push rebuilds its stack.  d_obs is stale afterwards — the host sequence is the reset path's: mw_snapshot_load, mw_render, then
 * mw_stack_refresh if a stack is set.  A record taken with a pending next-step reset restores an env whose next step installs its
 * next world; a record whose spare was consumed restores an env whose spare the next step's refill regenerates. */
int mw_snapshot_load(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count,
                     const uint8_t *d_snap, int32_t n_recs, int32_t capacity, void *stream);
/* Frame records, the opt-in companion of the state records: what the agent SAW, in a second caller-owned device buffer, so that a load
 * or fork can put the frames back instead of drawing them again.  A frame record holds
 *   - the env's row of d_obs as it stands at the save, in the layout of mw_set_obs_layout — whatever the row holds: the engine cannot
 *     know whether it is the env's current frame (after a step or render into d_obs it is);
 *   - with MW_SNAPF_DEPTH, its row of d_depth;
 *   - with MW_SNAPF_STACK, its `depth` stacked frames in WINDOW order, oldest first (mw_stack_window), and its stack flag byte ("rebuild
 *     on the next push": reset and not refreshed, or a next-step reset pending).  Window order does not depend on the ring position:
 *     a record is valid at any later push count and in another engine.
 *   the buffer  opaque, 16-byte aligned, mw_snapshot_frames_bytes(capacity, flags) bytes.  A 64-byte header carries a key — a format
 *               number, obs_width, obs_height, the obs layout, the bytes of a frame, flags, the stack depth, capacity —, the records
 *               follow record-major (a frame is contiguous), each section 16-byte aligned.  Compatible between engines of the same frame
 *               configuration in one process, whatever their num_envs.  It must not overlap d_obs, d_depth or the stack's ring.
 * Both calls are one kernel launch, asynchronous on `stream` and ordered there like any other call: a save behind a step sees that
 * step's frames and its push.  d_envs / d_recs as for the state records.
 * Errors.  MW_E_INVALID before anything is launched: a null engine, d_frames or d_obs; a misaligned d_frames; count < 0,
 * count > capacity, n_recs > capacity; count > num_envs on a load or on a save with d_envs == NULL; unknown flag bits; MW_SNAPF_DEPTH
 * with a null d_depth; MW_SNAPF_STACK without a frame stack or under another obs layout than the stack was set under.  On the device
 * every env and record index is tested and a load compares the key (flags included: a buffer is loaded with the flags it was saved
 * with): an offending item writes nothing and sets the status bit that mw_check reports as MW_E_INVALID. */
enum { MW_SNAPF_DEPTH = 1, MW_SNAPF_STACK = 2 };
/* bytes of a buffer for `capacity` frame records under `flags` (host value, no sync; < 0 on error: capacity < 0, unknown flag bits,
 * MW_SNAPF_STACK without a frame stack or under another obs layout than the stack was set under) */
int64_t mw_snapshot_frames_bytes(const mw_engine *e, int32_t capacity, int32_t flags);
/* frame record k (k < count <= capacity) := the frames of env d_envs[k]; d_envs == NULL: env k, count <= num_envs.  Writes the header.
 * Changes nothing in the engine. */
int mw_snapshot_save_frames(mw_engine *e, const int32_t *d_envs, int32_t count, const uint8_t *d_obs, const float *d_depth,
                            uint8_t *d_frames, int32_t capacity, int32_t flags, void *stream);
/* env d_envs[k]'s rows of d_obs / d_depth := frame record d_recs[k].  Targets are distinct, records may repeat.  With MW_SNAPF_STACK the
 * env's row of the ring is written so that it is exactly the row the env would have had it pushed the record's `depth` frames itself,
 * at the engine's current push count: window frame k goes to slot first + k (mw_stack_window's first slot) and to the mirror slot
 * `depth` away where that lies inside 0 .. 2 * depth - 2, so this window and every later one are right and the ring position does not
 * move; the env's flag byte := the record's (an env saved while still marked for a rebuild stays marked: its next push or
 * mw_stack_refresh rebuilds it as ever).  The host sequence of a restore that carries its frames is mw_snapshot_load, then
 * mw_snapshot_load_frames with the same index arrays — no mw_render, no mw_stack_refresh: the env's observation is the one its source
 * returned (a picked-up object's last appearance included, which a redraw of the restored state does not show) and its stack is its
 * source's.  Like every call that writes d_obs it drops the frame that frame reuse holds; the frame cache stays (no state changed). */
int mw_snapshot_load_frames(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count, const uint8_t *d_frames,
                            int32_t n_recs, int32_t capacity, int32_t flags, uint8_t *d_obs, float *d_depth, void *stream);
/* Level sets: a bank of records a step loop restarts finished envs from.  The reference has one way to choose the world an env plays
 * next, env.reset(seed=s) between episodes (miniworld.py:544-668; Procgen's num_levels / start_level and Prioritized Level Replay are
 * built on exactly that); here a level is a record of a freshly reset env — state, stream and spare in the state record, first
 * observation, depth and stack in the frame record — and restarting an env from it is two copies and no draw.  Four calls beside the
 * four above, which they leave as they are.
 * mw_snapshot_save_at / mw_snapshot_save_frames_at stand in for the append of a level or an archive cell to a Python list: a bank
 * larger than the engine is filled in chunks, and a running loop adds the states it reaches. */
/* record d_recs[k] := the complete state of env d_envs[k], k < count.  d_recs == NULL: record k (mw_snapshot_save);
 * d_envs == NULL: env k.  The records named must be distinct (caller's contract); every other record of the buffer
 * keeps what it held.  Writes the header. */
int mw_snapshot_save_at(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count,
                        uint8_t *d_snap, int32_t capacity, void *stream);
int mw_snapshot_save_frames_at(mw_engine *e, const int32_t *d_envs, const int32_t *d_recs, int32_t count,
                               const uint8_t *d_obs, const float *d_depth, uint8_t *d_frames,
                               int32_t capacity, int32_t flags, void *stream);
/* mw_snapshot_load_where / mw_snapshot_load_frames_where stand in for the reference loop's "if done: env.reset(seed=next_level)"
 * (scripts/benchmark.py:36-37), for every env at once and without the host learning which envs finished. */
/* for every env i < num_envs with d_mask[i] != 0: env i := record d_recs[i].  d_mask uint8[N], d_recs int32[N], both on
 * the device; d_recs[i] is not read where d_mask[i] == 0.  No count, no host value, no synchronisation.
 * One kernel launch each, asynchronous on `stream`, ordered behind the Maze's side-stream refills as mw_snapshot_load is; the key is
 * compared as a load compares it.  The grid is over all num_envs envs whatever the mask holds (a workgroup whose items are all
 * unmasked leaves after reading the mask), and num_envs may exceed capacity: records repeat, the list form's count <= capacity rule does
 * not apply.  A masked env whose record index is outside 0 .. n_recs - 1 is skipped — it writes nothing — and sets the status bit that
 * mw_check reports as MW_E_INVALID; an index under a zero mask byte is never an error.  MW_E_INVALID before anything is launched: a null
 * engine, mask, index array (record i for env i is what the list form is for) or buffer; a misaligned buffer; n_recs outside
 * 0 .. capacity; the frame twin's flag rules (mw_snapshot_load_frames).
 * For every env it writes mw_snapshot_load_where owes what mw_snapshot_load owes — the frame-clean byte cleared, the occlusion cache
 * of its geometry set invalidated, its stack flag byte marked as after mw_reset (plus the record's pending next-step reset) — and
 * nothing to any other env: it leaves the other envs' cached frames alone (mw_set_frame_cache).  Where mw_snapshot_load clears the
 * frame cache of every env, this call advances the cache epoch of each env it writes, on the device; the epoch is part of a cached
 * frame's key and of no record, so none of that env's cached frames can match again, and every other env keeps its cache.
 * Both _where calls drop the held frame of frame reuse (mw_set_frame_reuse), as mw_snapshot_load_frames does: the engine cannot know
 * that a record's frame shows the record's state.  The next step therefore draws every env it cannot serve from the frame cache; with
 * the cache on, a clean env is an ordinary cache hit.
 * mw_snapshot_load_frames_where writes the masked envs' rows of d_obs, of d_depth with MW_SNAPF_DEPTH, and their ring rows and flag
 * bytes with MW_SNAPF_STACK exactly as mw_snapshot_load_frames would, and touches no byte of any other env's rows. */
int mw_snapshot_load_where(mw_engine *e, const uint8_t *d_mask, const int32_t *d_recs, const uint8_t *d_snap,
                           int32_t n_recs, int32_t capacity, void *stream);
int mw_snapshot_load_frames_where(mw_engine *e, const uint8_t *d_mask, const int32_t *d_recs, const uint8_t *d_frames,
                                  int32_t n_recs, int32_t capacity, int32_t flags, uint8_t *d_obs, float *d_depth,
                                  void *stream);

/* ---- navigation fields ------------------------------------------------------- */
/* The shortest-path cost from every cell of a grid over each env's floor plan to a target, with the walls in the way, and the next
 * cell on the way down: what navigation suites around comparable simulators ship as geodesic distance and shortest-path follower.
 * The reference has no such call; its users run Dijkstra on the host over env.wall_segs.  The two predicates are the reference's own:
 * a cell is blocked where a circle of the agent's radius (+ margin) at its centre meets a wall, by the closest-point test of
 * intersect_circle_segs (math.py:30-62), and the cells a slot target is reached from are those where near(ent) (miniworld.py:965-975)
 * holds in the floor plane.
 *
 * The grid: gx x gz cells of side `cell`, origin (min_x, min_z) of the env's own extent; the centre of cell (j, i) is
 * (min_x + (i + 0.5) * cell, min_z + (j + 0.5) * cell).  A cell is BLOCKED when its centre lies beyond max_x or max_z, when the
 * distance from its centre to a collision segment is < agent_radius + margin, or — with MW_NAV_ENTITIES — when
 * sqrt(dx*dx + dz*dz) < agent_radius + radius(slot) + margin for a slot that is not MW_ENT_NONE, not carried and not the target slot.
 * SOURCES are the unblocked cells whose centre is closer (in x, z) than `reach` to the target: row i of d_target (double[N][3]; y is
 * not read) with params->reach, or — d_target NULL — the position of entity slot target_slot, with that slot's near() threshold
 * radius + agent_radius + 1.1 * max_forward_step (formed in float32 for a mesh entity, as near() forms it).  A move to one of the 8
 * neighbours costs 5 (straight) or 7 (diagonal; both cells the move passes between must be unblocked).
 * The field: uint16[N][gz][gx]; 0xFFFF a blocked cell, 0xFFFE an unblocked cell no path reaches (no source at all: every unblocked
 * cell — not an error), every other value the exact cost of the cheapest path.  The result does not depend on the kernel's schedule. */
#define MW_NAV_ENTITIES 1       /* flags: entities block cells too */
#define MW_NAV_JACOBI 2         /* flags: relax by whole-grid passes instead of directional sweeps (measurement only: the same field) */
#define MW_NAV_BLOCKED 0xFFFF
#define MW_NAV_UNREACHED 0xFFFE
#define MW_NAV_MAX_CELLS 32768  /* gx * gz: the grid lives in 64 KiB of LDS */
#define MW_NAV_GRID 4           /* flags: the field is mw_nav_build_grid's; mw_nav_query's waypoint at cost 0 is the cell's own centre */
#define MW_NAV_MAX_INFLATE 16   /* mw_nav_build_grid: the largest inflation radius in cells */
typedef struct mw_nav_params {
    double cell;            /* side of a cell, > 0 */
    double margin;          /* added to the agent's radius, >= 0.  For mw_nav_build_grid the WHOLE inflation radius in metres: the agent's
                             * radius is not added there (the caller's grid may already hold it) */
    double reach;           /* point targets only: > 0 */
    int32_t gx, gz;         /* cells along x and z, >= 1, gx * gz <= MW_NAV_MAX_CELLS */
    int32_t flags;          /* MW_NAV_* */
    int32_t target_slot;    /* 0 .. max_ents - 1 (read where d_target is NULL, checked always) */
} mw_nav_params;
/* mw_nav_build: rows of d_field for every env i with d_mask[i] != 0 (d_mask uint8[N] on the device, NULL = all); other rows are not
 * touched.  One kernel, one workgroup per env, asynchronous on `stream`, no host value read; it reads live arrays only and changes
 * nothing in the engine.  An env whose extent the grid does not cover (the centre of the first cell past the grid is not beyond max_x /
 * max_z), or one of whose costs would reach 0xFFFE, gets a row of 0xFFFF throughout and sets a status bit that the next mw_check
 * reports as MW_E_INVALID, once.  MW_E_INVALID before anything is launched: a null engine, params or field, cell <= 0, gx or gz < 1,
 * more than MW_NAV_MAX_CELLS cells, margin < 0, a target slot outside 0 .. max_ents - 1, reach <= 0 with point targets. */
int mw_nav_build(mw_engine *e, const mw_nav_params *params, const uint8_t *d_mask, const double *d_target, uint16_t *d_field, void *stream);
/* mw_nav_query: one thread per env, for the agents' positions (d_pos NULL) or row i of d_pos (double[N][3]; y is not read).  The
 * env's cell is floor((x - min_x) / cell), floor((z - min_z) / cell), clamped to the grid; if it is blocked, the lowest-cost unblocked
 * cell of its 3 x 3 neighbourhood stands in (0xFFFE counts as unblocked; ties: the first in the order below).  None, or a cell of
 * 0xFFFE: cost -1, next -1, the waypoint is the position itself.  Else
 *   d_cost[i]      int32, the cell's cost
 *   d_next[i]      int32, j * gx + i of the admissible neighbour of strictly lower cost with the lowest cost — ties go to the first in
 *                  the order (dj, di) = (-1,0), (1,0), (0,-1), (0,1), (-1,-1), (-1,1), (1,-1), (1,1) —, the cell itself at cost 0
 *   d_waypoint[i]  double[2], that cell's centre x, z; at cost 0 the target's x, z (d_target as for the build that made the field)
 * Any of the three outputs may be NULL.  The same argument checks as mw_nav_build.
 * With MW_NAV_GRID in params->flags (a field of mw_nav_build_grid) the waypoint at cost 0 is the centre of the cell itself, and neither
 * d_target nor target_slot is read; everything else is as above.  The descent ends on such a field too: with extra costs a cell's cost
 * still exceeds that of the neighbour it came through.  Without the flag the answers are what they were, bit for bit. */
int mw_nav_query(mw_engine *e, const mw_nav_params *params, const double *d_target, const uint16_t *d_field, const double *d_pos,
                 int32_t *d_cost, int32_t *d_next, double *d_waypoint, void *stream);
/* mw_nav_build_grid: the same field over the caller's own maps — a planner for a map an agent built from what it perceived (mw_depth_project's
 * obstacle plane, a seen map, anything rasterised by the caller), with several sources at once (the field is the cost to the nearest)
 * and a cost per cell.  It follows mw_nav_build where nothing else is said: one kernel, one workgroup per env, asynchronous on `stream`,
 * no host value read, nothing in the engine changes, rows of envs with d_mask[i] == 0 are not touched.  It reads only the caller's
 * tensors, and — with d_target alone — the env's extent for min_x, min_z.  Every grid is uint8[N][gz][gx] on the device, row-major like
 * the field, gx * gz bytes per env with no padding.  params: cell, gx, gz as before; reach for d_target; flags: MW_NAV_JACOBI is
 * honoured, MW_NAV_GRID accepted and ignored, MW_NAV_ENTITIES refused (this call reads no entities); target_slot is not read; margin
 * is the whole inflation radius in metres — the agent's radius is NOT added.
 *   BLOCKED   cell c is blocked when d_blocked[c] != 0 (a raw obstacle cell), and when some raw obstacle cell o at offset
 *             (dj, di) != (0, 0) from c has sqrt((double)(di*di + dj*dj)) * cell < margin: float64, in that order, strict, no
 *             contraction.  margin == 0 blocks the raw cells only.  The offsets run over |di|, |dj| <= R, R the smallest integer with
 *             R * cell >= margin.  Cells outside the grid hold no obstacle.  Nothing is blocked on account of the env's extent:
 *             the grid is the caller's, and mw_nav_build's refusal of a grid that does not cover the extent does not apply.
 *   SOURCES   an unblocked cell with d_sources[c] != 0, and — with d_target — the unblocked cells whose centre is closer than
 *             params->reach to row i of d_target (double[N][3], y not read), centres on the env's own min_x, min_z exactly as for
 *             mw_nav_build.  Either or both may be given, both give the union.  An env without any source: every unblocked cell
 *             0xFFFE, no error.
 *   COSTS     a source is 0, whatever d_extra says.  Every other unblocked cell c costs d_extra[c] (NULL: 0) plus the minimum over its
 *             admissible neighbours d of cost(d) + 5 (straight) or + 7 (diagonal, both cells the move passes between unblocked).
 *             The fixed point is unique; 0xFFFF and 0xFFFE mean what they mean above.
 * An env one of whose costs would reach 0xFFFE gets a row of 0xFFFF throughout and sets the status bit mw_nav_build sets: the next
 * mw_check reports MW_E_INVALID, once.  MW_E_INVALID before anything is launched: a null engine, params, d_blocked or d_field; both
 * d_sources and d_target null; cell <= 0, gx or gz < 1, more than MW_NAV_MAX_CELLS cells; margin < 0 or not finite, or R above
 * MW_NAV_MAX_INFLATE; MW_NAV_ENTITIES in flags; reach <= 0 with d_target.  With d_extra the kernel holds a byte per cell more in LDS
 * (at most 64 + 32 KiB). */
int mw_nav_build_grid(mw_engine *e, const mw_nav_params *params, const uint8_t *d_mask,
                      const uint8_t *d_blocked /* uint8[N][gz][gx]: != 0 a raw obstacle cell */,
                      const uint8_t *d_sources /* uint8[N][gz][gx] or NULL: != 0 a source cell */,
                      const double *d_target /* double[N][3] or NULL: point sources with params->reach */,
                      const uint8_t *d_extra /* uint8[N][gz][gx] or NULL: the extra cost of a cell */, uint16_t *d_field, void *stream);
/* measurements: d_passes, int32[N] on the device, gets the relaxation's count of rounds of every env each later mw_nav_build or
 * mw_nav_build_grid builds; NULL stops that */
int mw_debug_set_nav_passes(mw_engine *e, int32_t *d_passes);

/* ---- ray casts --------------------------------------------------------------- */
/* What a ray from a point of an env's floor plan meets first, and how far away: the range sensor ("lidar"), the line-of-sight test
 * and the free-path test of a disc that navigation suites around comparable simulators ship (Habitat's cast_ray, MuJoCo's mj_ray,
 * PyBullet's rayTestBatch).  The reference has no ray call; its users write one in numpy over env.wall_segs.  The obstacles and the
 * "starts inside" predicate are the reference's own: the collision segments and entity circles of
 * MiniWorldEnv.intersect (miniworld.py:937-963), the closest-point distance of intersect_circle_segs (math.py:30-62).
 *
 * Ray k of env i is o + t * d, t in [0, max_t]: o row [i][k] of d_origin (x, y, z; y is not read) or, d_origin NULL, the env's agent
 * position; d = (dx, dz) row [i][k] of d_dir, of any length, or, d_dir NULL, the fan: the angle agent_dir[i] + d_offsets[k] and
 * d = (cos, -sin) of it — the reference's dir_vec, through the same deterministic sin / cos as the dynamics (a NaN direction for an
 * angle of 1e6 or more in magnitude).  d_t[i][k] is the smallest such t at which the ray meets an obstacle, d_hit[i][k] says which:
 * the segment's index for a wall, MW_RAY_ENT + slot for an entity; where it meets none, d_t = max_t and d_hit = -1.  With unit
 * directions t is metres; with d = B - A and max_t = 1, "t < 1" says that something is in the way from A to B.  d_dir_out, if given,
 * receives the directions used, in either mode.
 *
 * Obstacles: the env's collision segments; with MW_RAY_ENTITIES also every slot whose kind is not MW_ENT_NONE and which is not the
 * carried one, as a circle of radius radius(slot) + params->radius (summed in float64) about its x, z.
 * All arithmetic is float64, + - * / and sqrt only, uncontracted, in this order (R: a circle's radius, r = params->radius):
 *   circle         w = o - c; A = dx*dx + dz*dz; B = wx*dx + wz*dz; C = (wx*wx + wz*wz) - R*R.  C < 0: t = 0.  Else disc = B*B - A*C;
 *                  disc < 0: no hit; else t = (-B - sqrt(disc)) / A, which counts when t >= 0
 *   segment a-b    e = b - a; den = dx*ez - dz*ex; den == 0 (parallel): no hit.  w = a - o; t = (wx*ez - wz*ex) / den;
 *                  s = (wx*dz - wz*dx) / den; counts when t >= 0 and 0 <= s <= 1 (both endpoints inclusive)
 *   wall, r == 0   the segment
 *   wall, r > 0    a capsule.  The closest-point distance from o to the wall < r: the ray starts inside, t = 0.  Else
 *                  len = sqrt(ex*ex + ez*ez), n = ((ez / len) * r, (-ex / len) * r), and t is the smallest of the circles of radius r
 *                  about a and b and of the segments (a + n)-(b + n) and (a - n)-(b - n)
 * A candidate counts only when t < best, from best = max_t (then best = t + 0.0), walls in index order, then slots in order: equal
 * t goes to the lowest code, and the result does not depend on how the work is spread over lanes.  Garbage is no error and no test
 * holds for a NaN: a NaN anywhere in a ray's origin or direction gives max_t and -1, a zero direction hits only what its origin is
 * inside, origins outside the extent are ordinary. */
#define MW_RAY_ENTITIES 1        /* flags: listed entities are obstacles too */
#define MW_RAY_ENT 0x10000       /* d_hit: MW_RAY_ENT + slot for an entity, the segment index for a wall, -1 for nothing */
#define MW_RAY_MAX 4096          /* rays per env and call */
typedef struct mw_ray_params {
    double max_t;                /* > 0, finite: rays are cut at o + max_t * d */
    double radius;               /* >= 0, finite: 0 a ray, > 0 a disc of this radius swept along it */
    int32_t rays;                /* R, 1 .. MW_RAY_MAX */
    int32_t flags;               /* MW_RAY_* */
} mw_ray_params;
/* All pointers are device pointers.  One kernel, asynchronous on `stream`, no host value read, no synchronisation; it reads live arrays
 * only and changes nothing in the engine.  d_mask: uint8[N] or NULL (all envs); rows of envs under a zero mask byte are neither read
 * (origins, directions) nor written.  MW_E_INVALID before anything is launched, and nothing touched: a null engine, params or d_t,
 * rays outside 1 .. MW_RAY_MAX, max_t not > 0 or not finite, radius < 0 or not finite, unknown flag bits, both or neither of d_dir /
 * d_offsets; also an engine whose max_segs and max_ents need more than 64 KiB of LDS at 48 bytes per segment and 32 per slot (rays >= 64 only). */
int mw_ray_cast(mw_engine *e, const mw_ray_params *params, const uint8_t *d_mask,
                const double *d_origin  /* [N][R][3] (y is not read) or NULL = the env's agent position for all its rays */,
                const double *d_dir     /* [N][R][2] = (dx, dz), any length, or NULL */,
                const double *d_offsets /* [R], radians, shared by all envs: the fan; exactly one of d_dir / d_offsets is non-null */,
                double *d_t /* [N][R] */, int32_t *d_hit /* [N][R] or NULL */, double *d_dir_out /* [N][R][2] or NULL */,
                void *stream);
/* measurements: form 1 casts every ray count with a ray per lane, 2 with an obstacle per lane (the same bits either way), 0 leaves the
 * choice to the ray count again */
int mw_debug_set_ray_form(mw_engine *e, int form);

/* ---- explored-area maps ------------------------------------------------------ */
/* Which cells of its floor plan each agent has seen so far, and how many of them are new: the coverage reward, the top-down map with
 * fog of war (Habitat's), the occupancy input of Active Neural SLAM style policies, the frontier of frontier exploration.  The
 * reference has no such call.  The map accumulates in the caller's tensor, like a nav field; the engine keeps nothing of it.
 *
 * The grid: a seen map is uint8[N][gz][gx], 0 unseen and 1 seen, on the grid of a nav field of the same cell, gx, gz — origin
 * (min_x, min_z) of the env's own extent, the centre of cell (j, i) at (min_x + (i + 0.5) * cell, min_z + (j + 0.5) * cell) — so that
 * map and field line up cell for cell.
 *
 * Sight: cell (j, i) of env e is VISIBLE in a call iff all of the following hold; all arithmetic is float64, + - * / and sqrt only,
 * uncontracted, in this order:
 *   1  its centre c is not beyond the extent (c.x > max_x or c.z > max_z, as a nav field's blocked border)
 *   2  with v = (cx - ox, cz - oz) from the agent's position o: dist = sqrt(vx*vx + vz*vz), and dist <= range
 *   3  cos_half == -1.0 (all round), or dist == 0.0, or vx*hx + vz*hz >= cos_half * dist, where h = (cos, -sin) of agent_dir — the
 *      reference's dir_vec, through the same deterministic sin / cos as the dynamics, as the fan of mw_ray_cast forms it for offset 0
 *   4  the line of sight is free: the ray with origin o, direction v, max_t = 1 and radius 0 meets nothing under exactly mw_ray_cast's
 *      arithmetic and rules, t == 1 and hit == -1.  The obstacles are the collision segments and, with MW_SEEN_ENTITIES, every slot
 *      whose kind is not MW_ENT_NONE and which is not the carried one, as its circle; a candidate counts only when t < 1, both endpoints
 *      of a segment are inclusive.
 * No test holds for a NaN: a NaN agent pose marks nothing.
 *
 * One call, for every env i with d_mask[i] != 0 (d_mask uint8[N] on the device, NULL = all): if d_clear[i] != 0 (uint8[N], NULL = none)
 * its row is zeroed and its count set to 0 first; then every visible cell is set to 1.  d_new[i] gets the number of cells that went
 * 0 -> 1 in this call, d_count[i] becomes (cleared ? 0 : d_count[i]) + d_new[i]: the count is carried, never recounted over the grid.
 * Rows, counts and d_new of envs under a zero mask byte are neither read nor written: the mask wins over clear.  Every cell has one
 * owner and the counts are integer sums, so the result does not depend on the kernel's schedule.  An env whose extent the grid does not
 * cover (as for mw_nav_build) gets its row zeroed, count 0 and new 0, and sets a status bit that the next mw_check reports as
 * MW_E_INVALID, once. */
#define MW_SEEN_ENTITIES 1       /* flags: listed entities block the line of sight too, as discs of full height */
/* One kernel, one workgroup per env, asynchronous on `stream`; it reads no host value except host_sight (during the call), reads live
 * arrays only and changes nothing in the engine.  MW_E_INVALID before anything is launched, and nothing touched: a null engine, grid,
 * host_sight, d_seen or d_count; cell <= 0, gx or gz < 1, more than MW_NAV_MAX_CELLS cells; a range that is not > 0 or not finite; a
 * cos_half outside -1 .. 1 or NaN; unknown flag bits; more workgroups than a launch holds; an engine whose max_segs and max_ents need
 * more than 64 KiB of LDS at 48 bytes per segment and 32 per slot beside the kernel's own 2064. */
int mw_seen_update(mw_engine *e, const mw_nav_params *grid /* cell, gx, gz are read; the rest is ignored */,
                   const double *host_sight /* [2] on the host, read during the call: range in metres, cos(fov / 2) or -1 */,
                   int32_t flags, const uint8_t *d_mask, const uint8_t *d_clear,
                   uint8_t *d_seen, int32_t *d_count, int32_t *d_new /* or NULL */, void *stream);

/* ---- egocentric map windows -------------------------------------------------- */
/* A small window of points centred on each agent and turned so that "up" is its heading: where walls and entities are, which points
 * the agent sees right now, and what a grid over the floor plan — a seen map, a nav field, the caller's own — holds there.  MiniGrid's
 * partial view, Habitat's ego_map sensor, the local map of Active Neural SLAM style policies and of local planners.  The reference
 * has no such call.
 *
 * The window: size = S, 1 .. MW_EGO_MAX_SIZE; row r = 0 is the farthest ahead, column c grows to the agent's right.  All arithmetic is
 * float64, + - * / floor and sqrt only, uncontracted, in this order:
 *   lat = (((double)c + 0.5) - (double)S * 0.5) * cell
 *   fwd = (((double)S * 0.5 - ((double)r + 0.5)) + back) * cell      back in cells: 0 the agent at the window's centre, S / 2 on the
 *                                                                    middle of its bottom edge
 *   the axes: f = (hx, hz) = (cos, -sin) of agent_dir — the reference's dir_vec through the same deterministic sin / cos as the dynamics,
 *   as the fan of mw_ray_cast forms it for offset 0 — and rt = (-hz, hx), the reference's right_vec; with MW_EGO_NORTH the constants
 *   f = (0, -1), rt = (1, 0): rows then grow with z and columns with x, like every grid here
 *   px = ox + (fwd * fx + lat * rtx), pz = oz + (fwd * fz + lat * rtz), o the agent's position or row i of d_pos (the heading is
 *   always the agent's)
 * The planes at point p, one uint8 each; every test is written so that a NaN fails it:
 *   MW_EGO_WALL     0 iff px >= min_x && px <= max_x && pz >= min_z && pz <= max_z (the env's extent) and the closest-point distance
 *                   from p to a collision segment (mw_nav_build's) is < wall_radius for no segment of the env; else 1.  A NaN pose: 1.
 *   MW_EGO_ENTITY   0, or 1 + the lowest slot whose kind is not MW_ENT_NONE, which is not the carried one and for which
 *                   dx*dx + dz*dz < R*R with d = p - its (x, z) and R = radius(slot) + entity_pad (summed in float64: mw_ray_cast's
 *                   circle under radius = entity_pad)
 *   MW_EGO_VISIBLE  tests 2 - 4 of mw_seen_update with p in the cell centre's place: v = p - o, dist <= range, the cone about the
 *                   agent's heading (with MW_EGO_NORTH too), the line of sight free under exactly mw_ray_cast's arithmetic with
 *                   max_t = 1 and radius 0 — walls, and with MW_EGO_ENTITIES the listed slots' circles
 * The sample (d_src given): fi = floor((px - min_x) / src_grid->cell), fj = floor((pz - min_z) / src_grid->cell); the point is inside
 * iff fi >= 0.0 && fi < (double)gx && fj >= 0.0 && fj < (double)gz, compared as doubles before any conversion; inside,
 * d_sample[i][r][c] = d_src[i][(int)fj][(int)fi], otherwise fill truncated to src_bytes.  No clamping, no status bit.  Elements are 1
 * byte (a seen map, the caller's own uint8 grid) or 2 (a nav field).
 * Rows of envs under a zero mask byte are neither read (d_pos) nor written.  Every cell has one owner, so the result does not depend
 * on the kernel's schedule. */
#define MW_EGO_ENTITIES 1        /* flags: listed entities block the line of sight of MW_EGO_VISIBLE too */
#define MW_EGO_NORTH 2           /* flags: the window keeps the world's axes instead of turning with the agent */
#define MW_EGO_WALL 1            /* planes */
#define MW_EGO_ENTITY 2
#define MW_EGO_VISIBLE 4
#define MW_EGO_MAX_SIZE 128
/* One kernel, one workgroup per env, asynchronous on `stream`; it reads no host value except host_window (during the call), reads live
 * arrays only and changes nothing in the engine.  MW_E_INVALID before anything is launched, and nothing touched: a null engine or
 * host_window; size outside 1 .. MW_EGO_MAX_SIZE; a cell that is not > 0 and finite; a back that is not finite; a wall_radius or
 * entity_pad < 0 or not finite; with MW_EGO_VISIBLE a range that is not > 0 or not finite, a cos_half outside -1 .. 1 or NaN; unknown
 * plane or flag bits; planes == 0 without a source; d_planes null while planes != 0; MW_EGO_ENTITY on an engine of more than 255 slots;
 * a source without src_grid, d_sample or src_bytes in {1, 2}, or whose grid mw_nav_build would refuse (cell <= 0, gx or gz < 1, more
 * than MW_NAV_MAX_CELLS cells); src_grid, d_sample or src_bytes != 0 without d_src is no error, they are ignored; more workgroups than
 * a launch holds; an engine whose max_segs and max_ents need more than 64 KiB of LDS for the asked planes (VISIBLE 48 bytes per
 * segment and 32 per slot, WALL 32 per segment, ENTITY 32 per slot). */
int mw_ego_map(mw_engine *e, const double *host_window /* [6] on the host: cell, back, wall_radius, entity_pad, range, cos_half */,
               int32_t size, int32_t planes, int32_t flags, const uint8_t *d_mask,
               const double *d_pos /* [N][3] (y is not read) or NULL = the agents */,
               uint8_t *d_planes /* [N][P][size][size]: P = popcount(planes) planes in bit order; NULL iff planes == 0 */,
               const mw_nav_params *src_grid /* cell, gx, gz are read */, const void *d_src /* [N][gz][gx] of src_bytes each or NULL */,
               int32_t src_bytes /* 1 or 2 with d_src */, uint32_t fill, void *d_sample /* [N][size][size] of src_bytes each */, void *stream);

/* ---- depth projection -------------------------------------------------------- */
/* The map a depth sensor gives: every pixel of each env's depth map — float32 [N][H][W], eye depth in metres, row 0 the top, what mw_step
 * and mw_render write with want-depth buffers: the reference's get_depth_map(0.04, 100), opengl.py:400-435 — is unprojected with the env's
 * own camera (cam_height, cam_fwd_disp, cam_pitch, cam_fov_y; miniworld.py:1200-1222, entity.py:477-503) and the pose the device holds
 * now, classed by its height as floor, obstacle or neither, and counted into a cell of an egocentric window laid out as mw_ego_map's or of
 * a grid over the floor plan laid out as mw_nav_build's.  Active Neural SLAM's mapper, Habitat's ego_map from depth, every "local map from
 * RGB-D" planner.  The privileged counterparts are mw_ego_map and mw_seen_update, computed from the collision segments: they are the labels
 * and the check of this one, which is what a policy without simulator state may consume.  The reference has no such call.
 *
 * All arithmetic is float64, only + - * /, floor and the engine's deterministic sin / cos (the one of the dynamics, mw_ray_cast's fan),
 * uncontracted, in exactly this order.  W x H is the engine's frame, pixel row v counts from the top, column u from the left.
 * Per env:
 *   o = the agent's (x, z); f = (hx, hz) = (cos, -sin) of agent_dir and rt = (-hz, hx), exactly mw_ego_map's axes
 *   (sp, cp) = sincos(pitch_deg * M_PI / 180.0); (sh, ch) = sincos(fov_deg * 0.5 * M_PI / 180.0); th = sh / ch
 *   aspect = (double)W / (double)H; tx = th * aspect
 * Per pixel:
 *   d = (double)depth[v][u]; the pixel is dropped unless d >= min_range && d <= max_range (so a NaN is dropped)
 *   xn = (((double)u + sub_x) * 2.0) / (double)W - 1.0
 *   yn = 1.0 - (((double)v + sub_y) * 2.0) / (double)H
 *   lat = (xn * tx) * d
 *   yc = (yn * th) * d
 *   fwd = fwd_disp + (d * cp - yc * sp)
 *   up = height + (d * sp + yc * cp)                 the height above the agent's own pos.y
 *   floor iff up >= -floor_tol && up <= floor_tol; obstacle iff up > floor_tol && up <= top; otherwise dropped (ceiling, sky)
 *   px = ox + (fwd * fx + lat * rtx); pz = oz + (fwd * fz + lat * rtz)
 * (sub_x, sub_y) is where in the pixel the engine took the depth: sample 0 of its multisample pattern, (sx, sy) / 16 in GL space with y up
 * — (9, 5) at 8 samples, (6, 2) at 4, (8, 8) at 1 —, so sub_x = sx / 16.0 and sub_y = 1.0 - sy / 16.0: not the pixel's centre.
 * The window target (grid == NULL; size = S, cell, back and MW_EGO_NORTH as in mw_ego_map, whose point (r, c) is the centre of cell (r, c)):
 *   a = lat, b = fwd; with MW_EGO_NORTH a = px - ox, b = -(pz - oz)
 *   c = floor(a / cell + (double)S * 0.5); r = floor(((double)S * 0.5 + back) - b / cell)
 *   the point is kept iff c >= 0.0 && c < (double)S && r >= 0.0 && r < (double)S, compared as doubles before any conversion
 *   d_planes[i][0][r][c] = min(255, the floor points of the cell), d_planes[i][1][r][c] = min(255, its obstacle points); both planes are
 *   written in full by every call.
 * The map target (grid != NULL: cell, gx, gz are read; min_x, min_z the env's own extent):
 *   fi = floor((px - min_x) / cell), fj = floor((pz - min_z) / cell); kept iff fi >= 0.0 && fi < (double)gx && fj >= 0.0 && fj < (double)gz
 *   (mw_ego_map's sample test); the cell is [(int)fj][(int)fi]
 *   d_map is uint8[N][2][gz][gx], plane 0 free (floor points), plane 1 obstacle.  For every env i with d_mask[i] != 0: if d_clear[i] != 0 its
 *   two planes are zeroed and its counts set to 0 first; then a byte that is 0 becomes 1 when the call's count for the cell reaches
 *   min_points; no call ever clears a byte except through d_clear.  d_new[i][k] gets the cells of plane k that went 0 -> 1 in this call,
 *   d_count[i][k] becomes (cleared ? 0 : d_count[i][k]) + d_new[i][k].  An env whose extent the grid does not cover (as for mw_nav_build) gets
 *   its planes zeroed, counts 0 and new 0, and sets a status bit that the next mw_check reports as MW_E_INVALID, once.
 * Rows of envs under a zero mask byte are neither read nor written: the mask wins over clear.  A count is a sum of ones, so the result
 * does not depend on the kernel's schedule.  Every test is written so that a NaN fails it.
 *
 * What the sensor cannot do.  The depth map is a function of a 16-bit depth value; one step of that value at eye depth z is
 * z * z * (far - near) / (far * near * 65535) metres with near = 0.04, far = 100: 3.8 mm at 3 m, 3.8 cm at 10 m.  Choose max_range well below the
 * far plane: at 8 m a step is 2.4 cm, a tenth of a 0.25 m cell.  The sky reads 100.0 and is dropped by any such max_range. */
#define MW_DEPTH_MAX_PIXELS 65535       /* W * H of the engine's frame: a cell's floor and obstacle counts share one 32-bit word in the kernel */
/* One kernel, one workgroup per env, asynchronous on `stream`; it reads no host value except host_params (during the call), reads live
 * arrays only and changes nothing in the engine.  MW_E_INVALID before anything is launched, and nothing touched: a null engine, host_params
 * or d_depth; a frame of more than MW_DEPTH_MAX_PIXELS pixels (a cell's two 16-bit counts could carry into each other); a min_range or
 * max_range that is not > 0 and finite, min_range > max_range; a floor_tol < 0 or not finite; a top < floor_tol or not finite; for a window
 * a size outside 1 .. MW_EGO_MAX_SIZE, a cell that is not > 0 and finite, a back that is not finite, flags other than MW_EGO_NORTH, a null
 * d_planes; for a map a null d_map or d_count, flags != 0, min_points outside 1 .. 255, a grid mw_nav_build would refuse (cell <= 0 or not
 * finite, gx or gz < 1, more than MW_NAV_MAX_CELLS cells) or one of more than 16384 cells (4 bytes of LDS per cell, 64 KiB: use a larger
 * cell); more workgroups than a launch holds. */
int mw_depth_project(mw_engine *e, const double *host_params /* [6] on the host: min_range, max_range, floor_tol, top, cell, back (the last two: window) */,
                     const float *d_depth /* [N][H][W] */, const uint8_t *d_mask,
                     int32_t size, int32_t flags, uint8_t *d_planes /* [N][2][size][size]; read with grid == NULL */,
                     const mw_nav_params *grid /* NULL = the window target; else cell, gx, gz are read */, int32_t min_points,
                     const uint8_t *d_clear /* or NULL */, uint8_t *d_map /* [N][2][gz][gx] */, int32_t *d_count /* [N][2] */,
                     int32_t *d_new /* [N][2] or NULL */, void *stream);

/* ---- label frames ----------------------------------------------------------------------------------------------------------------
 * What every pixel of an env's observation shows — the third sensor image beside colour and depth (a semantic / instance image) —, cast
 * on the device from the live world: the label of pixel (u, v) is what the ray from the env's camera through the pixel's depth sample
 * meets first.  The reference has no such call; it stands in for what its users write against env.entities and the GL matrices
 * (miniworld.py:1197-1221 gluPerspective and gluLookAt, entity.py:150-161 MeshEnt.render, entity.py:409-432 Box.render, entity.py:205-207
 * the frames' transform, objmesh.py:280-292, miniworld.py:512 GL_CULL_FACE).  The ray is parametrised by eye depth t, so t is directly
 * comparable with the depth output of mw_step / mw_render, whose own 16-bit steps it is free of.
 *
 * All arithmetic is float64, only + - * /, sqrt and the engine's deterministic sin / cos, uncontracted, in exactly this order (W x H the
 * engine's frame, pixel row v from the top, column u; the camera terms o, f, rt, sp, cp, th, tx and the sample (sub_x, sub_y) are
 * mw_depth_project's; a float is widened first):
 *   eye       ex = ox + fwd_disp * fx;  ey = agent_y + height;  ez = oz + fwd_disp * fz
 *   ray       xn = (((double)u + sub_x) * 2.0) / (double)W - 1.0;  yn = 1.0 - (((double)v + sub_y) * 2.0) / (double)H
 *             lat = xn * tx;  yt = yn * th;  up = sp + yt * cp;  fwd = cp - yt * sp
 *             dx = fwd * fx + lat * rtx;  dy = up;  dz = fwd * fz + lat * rtz;  the point at eye depth t is eye + t * d
 *             a NaN in the eye or in d: the pixel shows nothing
 * Candidates, in this order; a candidate t counts when near <= t && t <= far && t < best, from best = +infinity, and then best = t + 0.0:
 * equal t goes to the lowest code, a NaN fails every test.
 *   1. the static polygons of the env's geometry set in index order, code = the index.  A vertex is (x, y, z) = v[i]; under MW_POLY_XF,
 *      with (s, c) = sincos((double)xf[3] * M_PI / 180.0), it is ((c * x + s * z) + xf[0], y + xf[1], (c * z - s * x) + xf[2]).
 *        plane   a = V1 - V0, b = V2 - V0;  n = (ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx)
 *                k = ((nx * (V0x - ex) + ny * (V0y - ey)) + nz * (V0z - ez))
 *                den = ((nx * dx + ny * dy) + nz * dz); none unless den < 0 or den > 0;  t = k / den
 *        inside  p = (ex + t * dx, ey + t * dy, ez + t * dz); for every edge V_i -> V_(i + 1 mod nv), e = V_(i + 1) - V_i,
 *                m = (ny * ez - nz * ey, nz * ex - nx * ez, nx * ey - ny * ex), mc = ((mx * V_ix + my * V_iy) + mz * V_iz):
 *                ((mx * px + my * py) + mz * pz) - mc >= 0.0 — the edge itself counts, so two polygons that share it leave no hole
 *   2. the slots of kind MW_ENT_BOX in slot order, code = MW_RAY_ENT + slot: the oriented box of Box.render.  (s, c) = sincos(dir);
 *      q = eye - pos;  o = (c * qx - s * qz, qy, s * qx + c * qz);  l = (c * dx - s * dz, dy, s * dx + c * dz); per axis with lo .. hi =
 *      -sx / 2 .. sx / 2, 0 .. sy, -sz / 2 .. sz / 2:  l == 0: none unless o >= lo && o <= hi; else t1 = (lo - o) / l, t2 = (hi - o) / l,
 *      tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1, none unless tn <= tf; enter = the largest tn, leave = the smallest tf; a hit
 *      iff enter <= leave, and t = enter: the entry point.  (|dir| >= 1e6 or NaN, outside sincos' domain: the slot shows nothing.)
 *   3. the slots of kind MW_ENT_MESH in slot order, code = MW_RAY_ENT + slot:
 *      MW_LABEL_MESH_BOUNDS  the upright cylinder of the slot's radius R and height on its pos, side and caps: w = (ex - pos.x, ez - pos.z);
 *                A = dx * dx + dz * dz; B = wx * dx + wz * dz; C = (wx * wx + wz * wz) - R * R;  A == 0: none unless C <= 0; else
 *                disc = B * B - A * C, none unless disc >= 0, q = sqrt(disc), enter = (-B - q) / A, leave = (-B + q) / A; then the y axis
 *                as a box's with o = ey - pos.y, lo .. hi = 0 .. height; t = enter
 *      MW_LABEL_MESH_EXACT   the triangles of the slot's uploaded mesh: vertex (x, y, z) becomes, with (s, c) = sincos(dir), rx = c * x +
 *                s * z, rz = c * z - s * x, the point (pos.x + scale * rx, pos.y + scale * y, pos.z + scale * rz); plane and inside test
 *                as for a polygon of three vertices, but none unless den < 0: the reference draws with GL_CULL_FACE, a triangle seen from
 *                behind is not there.  The slot's t is the smallest of its triangles'.
 * Every slot whose kind is not MW_ENT_NONE counts, the carried one included: it is drawn, so it is labelled.  MW_ENT_FRAME slots are
 * drawn through the polygon list and labelled there.
 *
 * The outputs, device pointers, every one but d_class may be NULL:
 *   d_class       uint8[N][H][W]   MW_LABEL_NOTHING (sky), _FLOOR, _CEILING, _WALL, _FRAME, _BOX, _MESH.  A static polygon is a _FRAME with
 *                                  MW_POLY_ENTITY, else a _WALL with MW_POLY_QUAD, else a _FLOOR when the normal of its own vertices
 *                                  (az * bx - ax * bz above, before any transform) points up, > 0, else a _CEILING
 *   d_code        int32[N][H][W]   the code above, -1 for nothing
 *   d_depth       float32[N][H][W] the winning t rounded once, (float)far for nothing; mw_depth_project takes it
 *   d_ent_pixels  int32[N][E]      the pixels that show each slot
 *   d_ent_box     int32[N][E][4]   their bounding box u0, v0, u1, v1, inclusive; W, H, -1, -1 for a slot without a pixel
 * The result of a pixel is the minimum of (t, place in the order above) over all candidates: it does not depend on the kernel's schedule.
 * Rows of envs under a zero mask byte are neither read nor written. */
enum { MW_LABEL_NOTHING = 0, MW_LABEL_FLOOR = 1, MW_LABEL_CEILING = 2, MW_LABEL_WALL = 3, MW_LABEL_FRAME = 4, MW_LABEL_BOX = 5, MW_LABEL_MESH = 6 };
#define MW_LABEL_MESH_EXACT  0          /* flags: mesh slots as their own triangles */
#define MW_LABEL_MESH_BOUNDS 1          /* flags: mesh slots as their bounding cylinders */
#define MW_LABEL_UNPRUNED    2          /* flags, tests and measurements: every triangle against every pixel — the same bits, slower */
struct mw_label_params {
    double near, far;           /* the eye depths a hit may have: the frame's are 0.04 and 100 */
    int32_t flags, pad;         /* MW_LABEL_MESH_* */
};
typedef struct mw_label_params mw_label_params;
/* One kernel, one workgroup per env, asynchronous on `stream`; it reads no host value except params (during the call), reads live arrays
 * only and changes nothing in the engine.  MW_E_INVALID before anything is launched, and nothing touched: a null engine, params or d_class;
 * flags other than MW_LABEL_MESH_BOUNDS and MW_LABEL_UNPRUNED; a near or far that is not finite, near < 0 (the kernel orders t by its bits) or near >= far; a
 * frame so wide that not one row of it fits the kernel's 64 KiB of LDS beside the staged scene, or a scene of more than 61440 polygons per
 * set or 4095 entity slots (a pixel's code is kept in 16 bits there); more workgroups than a launch holds. */
int mw_label_frame(mw_engine *e, const mw_label_params *params, const uint8_t *d_mask, uint8_t *d_class, int32_t *d_code, float *d_depth,
                   int32_t *d_ent_pixels, int32_t *d_ent_box, void *stream);

/* ---- object maps ---------------------------------------------------------------------------------------------------------------------
 * Labelled pixels projected onto the maps a depth sensor gives: the semantic map of an ObjectNav stack (SemExp's category channels,
 * Habitat's semantic top-down map).  Every pixel of an env's label image — int32 [N][H][W], mw_label_frame's d_code or the caller's own
 * category image — is unprojected with its depth exactly as mw_depth_project unprojects it and carries its id into the cell it falls in, of
 * an egocentric window laid out as mw_ego_map's (cell for cell an entity plane's, and a depth window's) or of a grid over the floor plan laid
 * out as mw_nav_build's.  With mw_depth_project's map and mw_nav_build_grid a policy can find, reach and recognise a goal from sensor
 * images alone.  The reference has no such call.
 *
 * All arithmetic is float64, only + - * /, floor and the engine's deterministic sin / cos, uncontracted, in exactly mw_depth_project's
 * order: the camera terms and the sample position (sub_x, sub_y), the range test and the height classes, px / pz, the window bin and the
 * map bin are the ones defined there, by name.  Every test is written so that a NaN fails it.  Per pixel k:
 *   the pixel counts iff mw_depth_project would count it as floor or as obstacle and its bin lies inside the target
 *   id = code[k] - base, valid iff code[k] >= base && code[k] - base <= 254 (compared before the subtraction: nothing overflows)
 *   key = id where valid, else 0xFFFE: "seen, no object"
 *   a cell's key is the minimum of its pixels' keys, from 0xFFFF: "not seen by this frame".  The lowest id wins a shared cell; the result
 *   does not depend on the kernel's schedule.
 * base = MW_RAY_ENT makes ids the entity slots of mw_label_frame's d_code; base = 0 takes the caller's own image, negative values for none.
 * The window target (grid == NULL; size, cell, back and MW_EGO_NORTH as in mw_depth_project):
 *   d_plane[i][r][c] = 1 + key where key <= 254, else 0; the plane is written in full by every call.
 * The map target (grid != NULL: cell, gx, gz are read; min_x, min_z the env's own extent).  The last observation wins — objects here are
 * picked up, carried, dropped, and a health kit respawns.  For an env i under the mask:
 *   d_clear[i] != 0: every byte d_map[i][j][c] is rewritten, 1 + key where key <= 254, else 0
 *   otherwise a cell whose key is 0xFFFF keeps its byte and every other cell gets key <= 254 ? 1 + key : 0: a cell seen empty now forgets
 *   the object it held, a cell out of view keeps what it knew.
 * The per-object outputs, for every id q < ids over the whole map of the env after the update:
 *   n = the cells whose byte is 1 + q; si, sj = the integer sums of their column and row indices (exact, order-free, below 2^28)
 *   d_obj_cells[i][q] = n
 *   d_obj_pos[i][q] = (min_x + ((double)si / (double)n + 0.5) * cell, 0.0, min_z + ((double)sj / (double)n + 0.5) * cell), three quiet
 *   NaNs when n == 0.  Row q of [N][K][3], made contiguous, serves as the points of mw_nav_build, mw_nav_build_grid or mw_nav_query.
 * Rows of envs under a zero mask byte are neither read nor written: the mask wins over clear.  An env whose extent the grid does not cover
 * (as for mw_nav_build) gets its map zeroed, its cells 0 and its positions NaN, and sets a status bit that the next mw_check reports as
 * MW_E_INVALID, "mw_label_project refused an env", once.
 *
 * One kernel, one workgroup per env, asynchronous on `stream`; it reads no host value except host_params (during the call), reads live
 * arrays only and changes nothing in the engine.  MW_E_INVALID before anything is launched, and nothing touched: everything
 * mw_depth_project refuses for the same host_params, d_depth, size, flags and grid, a frame of more than MW_DEPTH_MAX_PIXELS pixels
 * included; a null d_code; a base < 0; ids outside 0 .. 255; a window with a null d_plane or ids > 0; a map with a null d_map, or with
 * ids > 0 and both per-object outputs null; a map of more than 16384 cells (a key of LDS per cell: use a larger cell). */
int mw_label_project(mw_engine *e, const double *host_params /* [6], mw_depth_project's */,
                     const float *d_depth /* [N][H][W] */, const int32_t *d_code /* [N][H][W] */, int32_t base,
                     const uint8_t *d_mask, int32_t size, int32_t flags, uint8_t *d_plane /* [N][size][size], window target */,
                     const mw_nav_params *grid /* NULL = window */, const uint8_t *d_clear, uint8_t *d_map /* [N][gz][gx] */,
                     int32_t ids /* K: 0 .. 255 */, int32_t *d_obj_cells /* [N][K] or NULL */, double *d_obj_pos /* [N][K][3] or NULL */,
                     void *stream);

/* ---- grid sight -------------------------------------------------------------- */
/* What a pose would see on the caller's OWN map: line of sight over a uint8 grid of the caller's — a depth map's obstacle plane, its
 * own raster —, from many candidate cells per env, summed against a weight plane: the gain term of frontier-based exploration and of
 * Active Neural SLAM's global policy ("standing there, how much of what I do not know would I see?"), a visibility polygon on an
 * occupancy grid.  The twin of mw_seen_update, which reads the simulator's walls from the agent's true position, as mw_nav_build_grid
 * is mw_nav_build's.  The reference has no such call.
 *
 * The rule.  All of it is defined on cells of a nav grid (cell, gx, gz) and is integer except the cone.
 *   A viewpoint is a cell A = (ja, ia), a target a cell B = (jb, ib); dx = ib - ia, dz = jb - ja.
 *   Occlusion: cell Q = (j, i) HIDES B from A iff opaque[Q] != 0, Q != A and Q != B, Q lies in the bounding box of A and B, and
 *       2 * |dx * (j - ja) - dz * (i - ia)| <= |dx| + |dz|
 *     — the segment between the two centres meets Q's closed square.  Closed on purpose: a line through a corner is blocked, so two
 *     opaque cells that touch only at a corner seal (with < in place of <=, (0, 0) sees (7, 7) through an anti-diagonal wall of single
 *     cells).  The rule is symmetric in A and B.  Per step along the major axis at most 3 cells satisfy it, so a walk costs at most
 *     3 * max(|dx|, |dz|) probes.
 *   Range and cone, float64, + - * and sqrt only, uncontracted, in this order: vx = (double)dx * cell, vz = (double)dz * cell;
 *     dist = sqrt(vx*vx + vz*vz); dist <= range; cos_half == -1.0 || dist == 0.0 || vx*hx + vz*hz >= cos_half*dist, where (hx, hz) is
 *     the heading mw_ray_cast's fan forms for the viewpoint's angle at offset 0 — test 2 and 3 of mw_seen_update with the viewpoint at
 *     a cell centre.  The grid's origin does not enter.
 *   B is SEEN from A iff range and cone hold and no Q hides it.  A sees itself; an opaque B is seen (its face is).
 * gain[env][v] is the sum over the seen B of weight[B], or their count without a weight plane, as int32; seen[env][B] = 1 for every B
 * that any viewpoint of the env sees — the call never clears it.  Counts are integer sums and the stores are idempotent, so nothing
 * depends on the kernel's schedule.
 *
 * The viewpoints.  With d_cells: `views` flat cell indices j * gx + i per env; a value outside 0 .. gx*gz - 1 is "no viewpoint": its
 * gain is 0 and it marks nothing.  Their headings are d_dirs, radians like agent_dir; d_dirs == NULL requires cos_half == -1.  With
 * d_cells == NULL, views must be 1: the viewpoint is the agent's own cell on the env's grid (origin min_x, min_z; a position outside
 * is clamped to the border, as mw_nav_query clamps it) and the heading is the agent's; a NaN pose is no viewpoint, and an env whose
 * extent the grid does not cover gets gain 0 and the status bit, exactly as in mw_seen_update.  Rows of envs under a zero mask byte
 * are neither read nor written. */
#define MW_SIGHT_MAX_VIEWS 256   /* viewpoints per env and call */
/* One kernel, one workgroup per env, asynchronous on `stream`; it reads no host value except host_sight (during the call), reads live
 * arrays only and changes nothing in the engine.  MW_E_INVALID before anything is launched, and nothing touched: a null engine, grid,
 * host_sight, d_opaque or d_gain; cell <= 0, gx or gz < 1, more than MW_NAV_MAX_CELLS cells; a range that is not > 0 or not finite; a
 * cos_half outside -1 .. 1 or NaN; views outside 1 .. MW_SIGHT_MAX_VIEWS; without d_cells, views != 1 or a d_dirs; with d_cells and
 * without d_dirs, a cos_half other than -1; more workgroups than a launch holds. */
int mw_grid_sight(mw_engine *e, const mw_nav_params *grid /* cell, gx, gz are read; the rest is ignored */,
                  const double *host_sight /* [2] on the host, read during the call: range in metres, cos(fov / 2) or -1 */,
                  int32_t views, const uint8_t *d_mask, const uint8_t *d_opaque /* [N][gz][gx] */, const uint8_t *d_weight /* or NULL */,
                  const int32_t *d_cells /* [N][views] flat j*gx+i, or NULL */, const double *d_dirs /* [N][views] or NULL */,
                  int32_t *d_gain /* [N][views] */, uint8_t *d_seen /* [N][gz][gx] or NULL */, void *stream);

/* ---- grid regions ------------------------------------------------------------ */
/* The connected regions of a byte mask on the caller's OWN map, each with its size, its centroid's sums and one cell of its own to go
 * to: what turns a mask of frontier cells into frontiers (Yamauchi's explorer, Active Neural SLAM's planner, explore_lite), the cells a
 * nav field can reach at all (its moves never cut a corner, so what it reaches is a 4-connected region), the specks of an obstacle
 * plane.  It reads nothing of the simulator.  The reference has no such call.
 *
 * The rule.  All of it is integer and defined on cells of a nav grid (gx, gz), flat index j * gx + i.
 *   A cell of d_member with a byte != 0 BELONGS to the mask.  Two member cells are JOINED when they are neighbours: with connectivity 4
 *     the four cells that share an edge; with connectivity 8 also the four that share a corner, unconditionally (no "both cells between
 *     free" rule as in a nav field's diagonal move).
 *   A REGION is a maximal joined set; its ROOT is its lowest flat index.  The regions of at least min_cells cells are QUALIFIED and are
 *     taken in the order of their roots (scan order, like OpenCV's connectedComponentsWithStats); the first K = max_regions of them are
 *     LISTED.
 *   count[env]      the number of qualified regions.  It may exceed K: then the caller knows the list is cut.
 *   size[env][k]    the cells of the k-th qualified region, 0 for k >= count.
 *   sum[env][k]     the sum of the rows j and the sum of the columns i of its cells, (0, 0) for none; each is at most 2^30.
 *   cell[env][k]    its REPRESENTATIVE, -1 for none: the cell of the region that minimises
 *                       (size * j - sum_j)^2 + (size * i - sum_i)^2
 *                   in 64-bit integers (each term is at most 2^60); ties go to the lowest flat index.  It is always a cell OF the region:
 *                   a frontier's centroid may lie in a wall, its representative is a frontier cell.  A row of cell is, unchanged, a row
 *                   of mw_grid_sight's d_cells (-1 is no viewpoint there): hence MW_REGION_MAX == MW_SIGHT_MAX_VIEWS.
 *   label[env][j][i]  0 for a cell outside the mask, k + 1 for a cell of the k-th listed region, -1 for a member cell of a region that is
 *                   not listed (too small, or beyond K).  int16, a type torch compares.
 * Every element of every given output row of an env under the mask is written; nothing of an env under a zero mask byte is read or
 * written.  The results are integers the rule defines, so nothing depends on the kernel's schedule. */
#define MW_REGION_MAX 256        /* listed regions per env and call (== MW_SIGHT_MAX_VIEWS) */
/* One kernel, one workgroup per env, asynchronous on `stream`; it reads no host value, nothing of the world, and changes nothing in the
 * engine.  MW_E_INVALID before anything is launched, and nothing touched: a null engine, grid, d_member, d_count, d_size or d_cell;
 * cell <= 0, gx or gz < 1, more than MW_NAV_MAX_CELLS cells; a connectivity other than 4 or 8; min_cells < 1; max_regions outside
 * 1 .. MW_REGION_MAX; more workgroups than a launch holds. */
int mw_grid_regions(mw_engine *e, const mw_nav_params *grid /* cell, gx, gz are read; the rest is ignored */,
                    int32_t connectivity /* 4 or 8 */, int32_t min_cells, int32_t max_regions /* K */, const uint8_t *d_mask,
                    const uint8_t *d_member /* [N][gz][gx] */, int32_t *d_count /* [N] */, int32_t *d_size /* [N][K] */,
                    int32_t *d_cell /* [N][K] */, int32_t *d_sum /* [N][K][2] or NULL */, int16_t *d_label /* [N][gz][gx] or NULL */,
                    void *stream);
/* tests and measurements: the launch shape of the tile and mesh kernels, which the engine otherwise takes from the batch size and from
 * constants — so that a small batch runs the loops that only a large one reaches (several tiles per wavefront, several items per
 * persistent worker).  Every frame is the same bits under every shape.  0 keeps a value as it is at the moment.
 *   waves_per_env    wavefronts per env of the tile kernels; must divide the raster grid's tile count (ceil(W / 16) * ceil(H / 4))
 *   mesh_tile_waves  wavefronts of the listed mesh tiles' launch, at least 8 (each draws the list of class b % n_xcc, n_xcc <= 8)
 *   ent_blocks       persistent workgroups of the mesh entity kernel, at least 8 (the same)
 *   slow_waves       wavefronts of the mesh slow-path kernel, at least 1
 * MW_E_INVALID, and nothing changed: a null engine, a negative value, a waves_per_env that does not divide the tile count,
 * mesh_tile_waves or ent_blocks of 1 .. 7.  Afterwards the next frame is drawn whole (no frame reuse across the call). */
int mw_debug_set_launch_shape(mw_engine *e, int waves_per_env, int mesh_tile_waves, int ent_blocks, int slow_waves);

/* checks the device-side status word (capacity overflows, items a snapshot call skipped; envs mw_set_state_where, mw_nav_build, mw_seen_update, mw_grid_sight, mw_depth_project or mw_label_project skipped
 * — these are reported first, by one check each, and then forgotten, the others by every check from then on); synchronises `stream` */
int mw_check(mw_engine *e, void *stream);

/* ---- measurement ------------------------------------------------------------- */
/* average duration (ms) of the dominant (raster) kernel and of the setup kernel over the launches since
 * the last call, measured with HIP events on the stream the kernels ran on; enables timing on first use.
 * reset > 0: from now on one launch in `reset` is bracketed with events (1 = every launch; recording on every
 * launch costs a few percent of the step rate); reset = 0: the default, one in 8; reset < 0 switches timing off.
 * `launches` is the number of launches measured.  Returns <0 on error. */
int mw_kernel_time_ms(mw_engine *e, int32_t reset, double *raster_ms, double *setup_ms, int64_t *launches);

/* Which raster kernels drew the last frame (the FrameBuffer half of render_obs, opengl.py:202-398) — so that a test can say
 * which code its fixtures exercised: MW_PATH_QUAD the quad kernel (mw_rasterq.hip: small scenes, 8 or 4 samples),
 * MW_PATH_QUAD_MESH the same for every tile no mesh entity can touch + the mesh-aware tile kernel for the others,
 * MW_PATH_TILE the tile kernels (mw_raster.hip: big scenes, MW_K2Q=0), MW_PATH_GENERIC the generic-resolution kernels
 * (other sample counts, frames 128 pixels wide or high and wider or higher (the tile and quad kernels' 24-bit edge coefficients), frames
 * beyond 128 x 96 pixels (W H > 12 288: their 32-bit edge sums), frames off the 16 x 4 grid
 * other than the ragged tile kernels' (8 samples, even H, no meshes), MW_GENERIC_RASTER=1); -1 before the first frame.  Frames off
 * the grid that the tile kernels draw report MW_PATH_TILE. */
/* The `info` dict of the envs' step() as device arrays, asynchronous on `stream` (either pointer may be NULL):
 *   d_health  int32[N]     CollectHealth: info["health"] (collecthealth.py:100)
 *   d_ent_pos double[N][3] position of entity slot `ent_slot`: TMaze / YMaze info["goal_pos"] = box.pos (tmaze.py:89, ymaze.py:125)
 * Values are those of the state the device holds: with MW_AUTORESET_SAME_STEP an env that just finished reports its new episode; with
 * MW_AUTORESET_NEXT_STEP it reports the finished one (its next step installs the new episode).
 * d_health on an engine whose task is not MW_TASK_COLLECT is MW_E_INVALID (there is no health array). */
int mw_get_info(mw_engine *e, int32_t *d_health, double *d_ent_pos, int32_t ent_slot, void *stream);
/* The same two values as they stood when each env's LAST FINISHED episode ended (collecthealth.py:100: the health that ended it;
 * tmaze.py:89 / ymaze.py:125: that episode's goal_pos = position of entity slot mw_config.goal_ent) — with MW_AUTORESET_SAME_STEP the step
 * kernel keeps them before it installs the next world (Gymnasium's `final_info` of a same-step vector env); with MW_AUTORESET_NEXT_STEP it
 * keeps them on the step that ends the episode (mw_get_info reports the same values until the next step).  Undefined for an env that
 * has not finished an episode yet; either pointer may be NULL; d_health needs MW_TASK_COLLECT. */
int mw_get_final_info(mw_engine *e, int32_t *d_health, double *d_goal_pos, void *stream);
/* MW_AUTORESET_NEXT_STEP: d_out uint8[N] (device), 1 = the env's last step ended its episode and its next step will install the next world
 * (ignoring its action; reward 0, term = trunc = 0) — what a replay buffer masks out.  Asynchronous on `stream`; all zeros in the other
 * modes. */
int mw_get_reset_pending(mw_engine *e, uint8_t *d_out, void *stream);

/* ---- frames that need not be drawn ------------------------------------------- */
/* A frame is a pure function of the env's state, and a step may leave that state as it was: a forward move into a wall or an entity,
 * a turn that the carried box blocks, a pickup or drop that finds nothing to do.  The step kernel compares the state it loaded with
 * the state it stores and keeps one byte per env, "frame clean": agent pose, carried slot and the carried entity's pose are bit for
 * bit the same, no entity leaves or has just left the list, no world was installed (auto-reset), the step was no next-step reset.
 * MW_TASK_COLLECT engines never set it (kits respawn behind the step kernel).
 *
 * mw_set_frame_reuse(e, 1) lets mw_step leave the rows of such envs in d_obs / d_depth undrawn.  Off by default.  With it on, the
 * caller promises exactly two things:
 *   1. the d_obs / d_depth it passes to consecutive mw_step calls are the same buffers, and
 *   2. it has not written to them in between.
 * The engine checks what it can: it remembers which buffers (pointers, output layout) hold every env's current agent-view frame, and a
 * step skips clean envs only when it is a plain step of the whole batch into exactly those.  A whole agent-view frame — mw_render, or
 * an mw_step that drew every env — makes its buffers the remembered ones, so mw_reset + mw_render + mw_step on one buffer skips from
 * the first step.  Every other frame draws every env and forgets the buffers: another pointer or layout, mw_render_top,
 * mw_render_view, both passes of a step with final observations (mw_set_final_obs), frames with mesh entities (always drawn in full),
 * and every frame of an engine created with experiment flags (MW_DEBUG_FLAGS != 0; read once by mw_create, like MW_K2Q and
 * MW_GENERIC_RASTER, so no toggle changes the raster path under a held frame).
 * So does every call that writes something a frame depends on: mw_reset, mw_set_state, mw_set_geometry, mw_set_gen_program,
 * mw_upload_texture, mw_upload_mesh, mw_set_obs_layout, mw_set_final_obs, mw_debug_set_mesh_frame_seq, mw_set_frame_reuse itself.
 * Observations, depth, rewards and flags are bit for bit what they are with reuse off.  What the engine cannot see is promise 2: a
 * caller that scribbles into d_obs between steps (in-place normalisation, say) keeps its scribbles in the rows of clean envs. */
int mw_set_frame_reuse(mw_engine *e, int32_t on);
/* d_out uint8[N] (device): the frame-clean bytes of the last mw_step, whether or not reuse is on — for tests, and for consumers that
 * want to skip their own per-frame work (an encoder need not run again on a frame that did not change).  Asynchronous on `stream`; all
 * zeros before the first step; 0 for every env that was given a new world in the step, with and without final observations. */
int mw_get_frame_clean(mw_engine *e, uint8_t *d_out, void *stream);

/* The frame cache: the engine keeps, per env, the last `slots` distinct frames a plain mw_step / mw_step_repeat drew (0 .. 8; 0, the
 * default, turns it off and frees the memory) and copies one of them instead of drawing when the env is back in the state that frame
 * shows: turn left then right, a move that a later one undoes.  A cached frame matches when its key does, byte for byte: the agent's
 * position and direction, the carried slot, the carried entity's position and direction, and a per-env epoch that the device
 * advances whenever anything else a frame shows changes — a world installed (auto-reset, mw_reset), an entity removed behind the last
 * frame, a pickup or a drop.  The copies are the engine's own, so unlike frame reuse nothing is promised about d_obs / d_depth: the
 * caller may pass other buffers on every step and write to them as it likes.  A clean env that frame reuse may not skip (another
 * buffer) is an ordinary hit.
 * Used by plain steps of the whole batch through the quad kernel (small scenes, frames on the 16x4 grid) in the uint8 HWC layout,
 * without mesh entities and experiment flags, never by MW_TASK_COLLECT; every other frame — renders, top views, the passes of a step
 * with final observations, the tile kernels' frames — neither reads nor fills nor invalidates it, and an engine whose frames take
 * another path holds the setting and no memory.  Every call that writes something a frame depends on drops every env's cached frames
 * (one asynchronous clear of the key table in front of the next step that uses the cache): mw_reset, mw_set_state, mw_set_geometry,
 * mw_set_gen_program, mw_upload_texture, mw_upload_mesh, mw_set_obs_layout, mw_snapshot_load, mw_set_frame_cache itself, and a
 * change between steps with and without d_depth.
 * Memory: num_envs x slots x H x W x 3 bytes (59 MB per slot at 4096 envs of 80x60), plus num_envs x slots x H x W x 4 for the
 * depth maps once a step asks for depth (78 MB more per slot).  Observations, depth, rewards and flags are bit for bit what they are
 * with the cache off.  A drawn frame costs one more store of its bytes, so a policy that never revisits a state pays without gain. */
int mw_set_frame_cache(mw_engine *e, int32_t slots);
/* d_out uint8[N] (device): where each env's frame of the last plain mw_step came from — 0 drawn, 1 left alone as clean (frame reuse),
 * 2 + j copied from slot j of the frame cache.  The step kernel stores 0, the frame plan in front of the quad kernel the rest: zeros on the other raster paths.  Asynchronous on `stream`. */
int mw_get_frame_source(mw_engine *e, uint8_t *d_out, void *stream);
/* Test and diagnosis call (synchronises `stream`; the step path itself never does, and stays capturable): the frame plan the last
 * planned frame was drawn from — the plain whole-batch steps through the quad kernel with frame reuse or the frame cache on — copied
 * to the host with the cost inputs it was built from.  host_plan: the block, uint32[words]; words must be 96 + 9 N for N <= 65535
 * envs (an ordered plan) and 96 + 2 N beyond.  [0] draw entries, [1] copy entries, [2] 8 in an ordered plan and 0 otherwise,
 * [32..33] and [64..65] the entries of cost classes 0..3 and 4..7, 16 bits each, the lowest class in the lowest bits; from [96] N
 * places for copy entries env | slot << 24; from [96 + N] the draw entries env | victim slot << 24 — ordered: N places per cost
 * class, class 0 first; else one list.  The quad kernel's workgroups take the draw entries from the highest class down, then the
 * copies.  host_lengths: int32[N], the display-list length of every env in the last frame; an env's cost class is min(7, length / 4).
 * MW_E_INVALID before the first planned frame. */
int mw_get_frame_plan(mw_engine *e, uint32_t *host_plan, int64_t words, int32_t *host_lengths, void *stream);
/* Test and diagnosis call (synchronises `stream`): host_out uint8[N], 1 where the geometry kernel of the last planned frame built the
 * env's display list, 0 where it left it alone.  In front of a frame plan the geometry kernel of a small scene builds only the envs
 * the plan will have drawn, and those whose picked-up entity still has to leave the list, and deals them evenly over its wavefronts;
 * every env whose source byte says drawn was built.  An engine created with MW_GEOM_DEAL=0 in the environment builds every env on
 * every frame and never writes these bytes (zeros); they tell nothing of frames without a plan, which build every env. */
int mw_get_geom_built(mw_engine *e, uint8_t *host_out, void *stream);

/* Diagnostic (synchronises `stream`): how many triangles the last frame's display list held per env after clipping and culling —
 * what max_visible has to pay for (6 records per unit), and what decides which raster kernel an env's frame takes.
 * The stored length is clamped to the list's capacity (6 x max_visible): a value EQUAL to the capacity means "at least this
 * many" — raise max_visible and look again (mw_check reports the overflow itself as MW_E_CAPACITY).
 * An env that a planned frame did not build (mw_get_geom_built: 0) keeps the length — like the header and the records — of its last
 * build: the length of the frame that is on display only where that frame was drawn. */
int mw_get_list_lengths(mw_engine *e, int32_t first_env, int32_t count, int32_t *host_out, void *stream);

/* Test hook: the sequence number of the next frame with mesh entities.  Its low 16 bits stamp the per-pixel chains of the
 * fragments of mesh triangles that cross a frustum plane (a head of another stamp reads as empty; the heads are wiped on the
 * frame whose stamp is 0); a test moves it to the wrap instead of rendering 65 536 frames.  The parity must stay (the frame's
 * work lists alternate with it). */
int mw_debug_set_mesh_frame_seq(mw_engine *e, uint32_t seq);
/* ... and the chain heads themselves, uint32[N][H][W] = stamp << 16 | newest fragment of the pixel + 1 (synchronises `stream`). */
int mw_debug_get_slow_heads(mw_engine *e, uint32_t *host_out, void *stream);

enum { MW_PATH_TILE = 0, MW_PATH_QUAD = 1, MW_PATH_QUAD_MESH = 2, MW_PATH_GENERIC = 3 };
int mw_raster_path(const mw_engine *e);

#ifdef __cplusplus
}
#endif
#endif
