/* rtp_mesh.h -- mesh scenes: quad meshes of any size behind a BVH in the path
 * kernel.  Additions to the C ABI of rtp.h (RTP_ABI_VERSION stays 3); the
 * functions are exported from librtp.so like those of rtp.h. */
#ifndef RTP_MESH_H
#define RTP_MESH_H
#include "rtp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A mesh scene: the same descriptor with any number of quads from 1 to 2^22
 * (rtp_set_scene holds at most 256 distinct quads inline).  The quads are kept
 * in global memory behind a BVH that the path kernel walks -- always, also
 * for 18 quads -- and at most 8 spheres are scanned inline; with 9 or more
 * spheres the call returns RTP_ERR_INVALID_ARGUMENT (no quad BVH together
 * with a sphere BVH).  Ids, materials, the light quad and the light sphere are
 * checked as by rtp_set_scene, with its messages.  A refused call leaves the
 * previous scene in place; rtp_set_scene replaces a mesh scene and the other
 * way round.  Duplicate quads are kept: a later copy never wins.
 *
 * The closest hit is unchanged: the minimum of (t, quads before spheres, index
 * in the caller's list) over the hits with t > 0.001, every quad tested with
 * the general float32 arithmetic.  The boxes only cull, and the promise has a
 * limit like the sphere BVH's: the walk equals the brute-force scan for every
 * ray (a) whose origin lies within `reach` -- 2 diagonals of the scene's
 * bounding box -- of the vertices of the quad the scan reports, and (b) that
 * meets that quad's first-triangle plane (v00, v10, v01) with |cos(theta)| >=
 * cos_min = 2^-8, theta the angle to the plane's normal.  Outside it (origins
 * far away, rays within 0.22 degrees of the plane) the float32 test accepts
 * points arbitrarily far from the quad, and the walk may miss what the scan
 * would report.  rtp_mesh_guarantee returns cos_min and reach of the current
 * mesh scene.  (csrc/rtp_layout.hpp kMeshCosMin.)
 *
 * Bent quads and triangle cells.  A quad whose third vertex v11 is off the
 * first triangle's plane by 1/512 or more of its distance beyond the diagonal
 * gets an unbounded box, because the reference's test accepts such a quad
 * arbitrarily far away: always tested, sound, slow -- a mesh made mostly of
 * such quads renders as slowly as a brute-force scan, and a curved surface
 * given as quads is such a mesh.  Give it as triangles.  A triangle cell is a
 * cell whose v11 and v01 compare equal in all three coordinates, in
 * particular (a, b, c, c): the same point named as third and fourth id, the
 * usual way to state a triangle in a quad list.  Its meaning is what the
 * reference makes of that quad -- exactly its first triangle (v00, v10, v01)
 * with the normal of (v00, v10, v11 = v01), same closest hit, tie-break and
 * pixels -- and it always gets a tight box: its three vertices and a pad that
 * depends on the corner at v00 alone (unbounded only for a corner whose sine
 * is below 2^-10 or a pad beyond the reach).  A triangle costs one box, one
 * record and one test, like a planar quad (a 16 384-cell curved terrain as
 * 32 768 triangles: 12 ms a frame where its bent quads take 3.5 s, DESIGN.md
 * 4.11).  So split the bent quads of a mesh: (v00, v10, v11, v01) becomes (v00, v10,
 * v01, v01) and (v11, v01, v10, v10), both with the quad's orientation.  The
 * two halves are not the reference's bent quad: each reports t on its own
 * plane and accepts nothing beyond its edges -- which is the point.
 * rtp_mesh_counts reports the cells, the triangle cells among them and the
 * cells with an unbounded box of the current mesh scene (each output
 * optional): n_unbounded says why a mesh is slow.  It fails with
 * RTP_ERR_INVALID_ARGUMENT when the context holds no mesh scene.
 *
 * On a mesh scene rtp_render, rtp_render_device (range and pixel list; work
 * stealing), rtp_render_pixels, rtp_render_resume*, rtp_render_views* (the
 * per-view loop), rtp_debug_closest_hit and rtp_debug_bounce work.  Refused
 * with RTP_ERR_INVALID_ARGUMENT, nothing launched: rtp_render_tiles_device,
 * rtp_render_planned_device, rtp_render_guides* (and the denoised preview),
 * rtp_render_direct*, and every render under RTP_KERNEL=1 or
 * RTP_DEBUG_STATS=1.  RTP_MESH_SCAN=1 (read by this call) makes every render
 * of the scene scan all its quads instead of walking: the A/B handle. */
rtp_status rtp_set_scene_mesh(rtp_context* ctx, const rtp_scene_desc* scene);
rtp_status rtp_mesh_guarantee(rtp_context* ctx, float* cos_min, float* reach);
rtp_status rtp_mesh_counts(rtp_context* ctx, int32_t* n_cells, int32_t* n_triangles, int32_t* n_unbounded);

/* The same scene from arrays that already live on the context's device, for
 * cell sets a simulation moves every time step: `points`, `quad_points`,
 * `quad_mat` and `quad_tex` of the descriptor are DEVICE pointers; everything
 * else (the spheres' arrays, mat_type, tex_type, tex_rgb, the light ids, ior)
 * is host memory as before.  Limits, checks and messages are those of
 * rtp_set_scene_mesh -- the per-quad checks run on the device, and the first
 * failure by quad index decides the message -- and a refused call leaves the
 * previous scene in place and rendering.  The BVH (a linear BVH over the
 * quads' Morton codes), the quad records and the boxes are built on the
 * device; the host reads back the at most 13 points the spheres and lights
 * name, one 64-byte record and the node count, nothing that grows with the
 * mesh.  The work is enqueued on `hip_stream` (NULL: the null stream), behind
 * whatever the caller queued there to produce the arrays, and the call
 * returns once the scene is in place: it synchronises that stream.  The
 * caller's arrays are not kept.  The closest hit, the promise and
 * rtp_mesh_guarantee (the same cos_min and reach, bit for bit) are those of
 * rtp_set_scene_mesh for the same scene, and so is every pixel; only the
 * tree, and with it the walk's speed, differs.  RTP_MESH_SCAN=1 is honoured.
 * RTP_MESH_BUILD=gpu makes rtp_set_scene_mesh upload its host arrays and take
 * this path (the A/B handle); unset or `host`, it builds on the host. */
rtp_status rtp_set_scene_mesh_device(rtp_context* ctx, const rtp_scene_desc* scene, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RTP_MESH_H */
