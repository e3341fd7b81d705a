// Prints the layout of every struct of include/rtp.h that the ctypes binding
// mirrors, for the check of tests/test_progressive_api.py: one line per
// struct -- its name, its size, then name=offset per field in declaration
// order.  Header only: links nothing.
#include <cstddef>
#include <cstdio>

#include "rtp.h"

#define STRUCT(T) std::printf("\n" #T " %zu", sizeof(T))
#define FIELD(T, f) std::printf(" " #f "=%zu", offsetof(T, f))

int main() {
  STRUCT(rtp_camera);
  FIELD(rtp_camera, position), FIELD(rtp_camera, look_at), FIELD(rtp_camera, view_up), FIELD(rtp_camera, fov_y_deg);
  STRUCT(rtp_view);
  FIELD(rtp_view, camera), FIELD(rtp_view, seed_base);
  STRUCT(rtp_scene_desc);
  FIELD(rtp_scene_desc, points), FIELD(rtp_scene_desc, n_points), FIELD(rtp_scene_desc, quad_points);
  FIELD(rtp_scene_desc, quad_mat), FIELD(rtp_scene_desc, quad_tex), FIELD(rtp_scene_desc, n_quads);
  FIELD(rtp_scene_desc, sphere_point), FIELD(rtp_scene_desc, sphere_radius), FIELD(rtp_scene_desc, sphere_mat);
  FIELD(rtp_scene_desc, sphere_tex), FIELD(rtp_scene_desc, n_spheres), FIELD(rtp_scene_desc, mat_type);
  FIELD(rtp_scene_desc, n_mat), FIELD(rtp_scene_desc, tex_type), FIELD(rtp_scene_desc, n_tex_type);
  FIELD(rtp_scene_desc, tex_rgb), FIELD(rtp_scene_desc, n_tex), FIELD(rtp_scene_desc, light_quad_points);
  FIELD(rtp_scene_desc, light_sphere_point), FIELD(rtp_scene_desc, ior);
  STRUCT(rtp_stats);
  FIELD(rtp_stats, samples), FIELD(rtp_stats, live_bounces), FIELD(rtp_stats, nan_pixels), FIELD(rtp_stats, kernel_ms);
  STRUCT(rtp_pixel_aux);
  FIELD(rtp_pixel_aux, final_seed), FIELD(rtp_pixel_aux, live_bounces);
  STRUCT(rtp_render_state);
  FIELD(rtp_render_state, rgba), FIELD(rtp_render_state, seed), FIELD(rtp_render_state, live_bounces);
  FIELD(rtp_render_state, m2);
  STRUCT(rtp_direct_desc);
  FIELD(rtp_direct_desc, clip_near), FIELD(rtp_direct_desc, clip_far), FIELD(rtp_direct_desc, background);
  FIELD(rtp_direct_desc, composite_background), FIELD(rtp_direct_desc, quad_scalar), FIELD(rtp_direct_desc, color_map);
  FIELD(rtp_direct_desc, color_map_size);
  STRUCT(rtp_denoise_params);
  FIELD(rtp_denoise_params, levels), FIELD(rtp_denoise_params, sigma_l), FIELD(rtp_denoise_params, sigma_z);
  FIELD(rtp_denoise_params, sigma_a), FIELD(rtp_denoise_params, normal_log2);
  STRUCT(rtp_ff_info);
  FIELD(rtp_ff_info, policy), FIELD(rtp_ff_info, built), FIELD(rtp_ff_info, chain_tables);
  FIELD(rtp_ff_info, direct_first), FIELD(rtp_ff_info, direct_count), FIELD(rtp_ff_info, bytes);
  FIELD(rtp_ff_info, alloc_ms), FIELD(rtp_ff_info, build_ms), FIELD(rtp_ff_info, samples_seen);
  FIELD(rtp_ff_info, auto_samples), FIELD(rtp_ff_info, auto_samples_direct);
  std::printf("\n");
  return 0;
}
