// The structs of include/mwengine.h as the C++ compiler lays them out: tests/test_abi_mirror_cpu.py compares them with the ctypes
// classes of miniworld_amd/engine.py, member for member.  Prints one line per struct ("struct <name> <sizeof>") and one per member
// ("member <struct> <name> <offsetof> <size>"), the members in the header's order (the test checks that none is left out here).
#include <cstddef>
#include <cstdio>

#include "../../include/mwengine.h"

#define S(T) std::printf("struct %s %zu\n", #T, sizeof(T))
#define M(T, m) std::printf("member %s %s %zu %zu\n", #T, #m, offsetof(T, m), sizeof(((T *)0)->m))

int main()
{
    S(mw_range);
    M(mw_range, def); M(mw_range, lo); M(mw_range, hi);

    S(mw_config);
    M(mw_config, abi_version); M(mw_config, device_id); M(mw_config, num_envs); M(mw_config, obs_width); M(mw_config, obs_height);
    M(mw_config, msaa); M(mw_config, max_ents); M(mw_config, max_polys); M(mw_config, max_segs); M(mw_config, max_visible);
    M(mw_config, shared_geometry); M(mw_config, task); M(mw_config, goal_ent); M(mw_config, goal_ent2); M(mw_config, num_objs);
    M(mw_config, max_episode_steps); M(mw_config, domain_rand); M(mw_config, generator); M(mw_config, autoreset);
    M(mw_config, agent_radius); M(mw_config, agent_height); M(mw_config, max_forward_step);
    M(mw_config, forward_step); M(mw_config, forward_drift); M(mw_config, turn_step);
    M(mw_config, sky_color); M(mw_config, light_pos); M(mw_config, light_color); M(mw_config, light_ambient); M(mw_config, obj_color_bias);
    M(mw_config, cam_height); M(mw_config, cam_fwd_disp); M(mw_config, cam_pitch); M(mw_config, cam_fov_y);
    M(mw_config, gen_args); M(mw_config, gen_tab); M(mw_config, gen_colors);
    M(mw_config, tex_nvar); M(mw_config, tex_var_id); M(mw_config, tex_var_scale);
    M(mw_config, room_wall_height); M(mw_config, room_no_ceiling); M(mw_config, rng_mode);

    S(mw_poly);
    M(mw_poly, v); M(mw_poly, uv); M(mw_poly, n); M(mw_poly, nv); M(mw_poly, tex); M(mw_poly, rgb); M(mw_poly, xf);

    S(mw_state_view);
    M(mw_state_view, agent_pos); M(mw_state_view, agent_dir); M(mw_state_view, cam); M(mw_state_view, light); M(mw_state_view, carrying);
    M(mw_state_view, step_count); M(mw_state_view, num_picked_up); M(mw_state_view, ent_kind); M(mw_state_view, ent_mesh);
    M(mw_state_view, ent_static); M(mw_state_view, ent_pos); M(mw_state_view, ent_dir); M(mw_state_view, ent_geom); M(mw_state_view, extent);

    S(mw_prog_room);
    M(mw_prog_room, nverts); M(mw_prog_room, wall_tex); M(mw_prog_room, floor_tex); M(mw_prog_room, ceil_tex);
    M(mw_prog_room, ox); M(mw_prog_room, oz); M(mw_prog_room, nx); M(mw_prog_room, nz);
    M(mw_prog_room, min_x); M(mw_prog_room, max_x); M(mw_prog_room, min_z); M(mw_prog_room, max_z); M(mw_prog_room, cdf);

    S(mw_prog_op);
    M(mw_prog_op, op); M(mw_prog_op, slot); M(mw_prog_op, room); M(mw_prog_op, cond); M(mw_prog_op, dir_mode); M(mw_prog_op, flags);
    M(mw_prog_op, lx); M(mw_prog_op, hx); M(mw_prog_op, lz); M(mw_prog_op, hz); M(mw_prog_op, dir); M(mw_prog_op, a); M(mw_prog_op, b);

    S(mw_gen_program);
    M(mw_gen_program, n_rooms); M(mw_gen_program, n_tex); M(mw_gen_program, n_ops); M(mw_gen_program, n_ents); M(mw_gen_program, rooms);
    M(mw_gen_program, tex_nvar); M(mw_gen_program, tex_var_id); M(mw_gen_program, tex_var_scale); M(mw_gen_program, ops);
    M(mw_gen_program, ent_kind); M(mw_gen_program, ent_mesh); M(mw_gen_program, ent_static);
    M(mw_gen_program, ent_pos); M(mw_gen_program, ent_dir); M(mw_gen_program, ent_geom);
    M(mw_gen_program, colors); M(mw_gen_program, extent); M(mw_gen_program, street);
    M(mw_gen_program, sign_n); M(mw_gen_program, pad); M(mw_gen_program, sign_slot); M(mw_gen_program, sign_reward);

    S(mw_plan_trace);
    M(mw_plan_trace, agent_pos); M(mw_plan_trace, agent_dir); M(mw_plan_trace, carrying); M(mw_plan_trace, ent_pos); M(mw_plan_trace, ent_slot);

    S(mw_nav_params);
    M(mw_nav_params, cell); M(mw_nav_params, margin); M(mw_nav_params, reach); M(mw_nav_params, gx); M(mw_nav_params, gz);
    M(mw_nav_params, flags); M(mw_nav_params, target_slot);

    S(mw_ray_params);
    M(mw_ray_params, max_t); M(mw_ray_params, radius); M(mw_ray_params, rays); M(mw_ray_params, flags);
    return 0;
}
