/*
 * hybkf_group.h -- C ABI of slab groups (libhybkf_group.so): one native owner of N z-slab contexts that runs the per-frame
 * collective sequence of the slab merge itself, over RCCL or on one device.
 *
 * A group holds `members` kf_ctx, member i owning voxel layers [z_cuts[i], z_cuts[i+1]) plus a halo on each side (KF_GROUP_RCCL_RANK: the one
 * member owns [z_cuts[0], z_cuts[1]), this rank's slab of the world's layout).  Per frame and
 * member, kf_group_frame enqueues what pipeline.SlabPipeline runs with replicated ICP and speculative normals:
 *   1. depth in          a host frame is copied once per device into a group-owned buffer; kf_set_depth_mm_device
 *   2. kf_preprocess     (trunc_min, trunc_max, sigma_pixel, sigma_depth)
 *   3. kf_icp_track      every member tracks the whole image (replicated: the same pose bits everywhere); from here on the
 *                        device-resident pose (NULL transform), so a lost frame is handled on the device
 *   4. kf_integrate_volume           own layers + halo
 *   5. kf_raycast_volume_slab_cross_spec
 *   6. MIN all-reduce of the 64-bit crossing words
 *   7. kf_slab_ray_normals_spec
 *   8. integer SUM all-reduce of the 3-word normal candidates
 *   9. kf_set_model_maps_rays        -> every member holds the merged model maps (and levels 1, 2 of their pyramids)
 * A COLOUR group (kf_group_create_color, base->has_color = 1; frames through kf_group_frame_color / kf_group_frame_members_color) runs the same nine
 * steps in their colour forms, still with two collectives:
 *   1. depth and BGR in   the BGR frame is copied once per device like the depth frame; kf_set_rgb_device
 *   4. kf_integrate_volume(has_color = 1, use_angle_weight_color)   (colour excludes deferred weights: the plain fusion kernel at every size)
 *   5. kf_raycast_volume_slab_cross_spec_color     4 speculative words per pixel: the normal, then the colour at the vertex
 *   7. kf_slab_ray_normals_color                   the vertex's owner contributes normal AND colour (a pixel without a normal may have a colour)
 *   8. integer SUM all-reduce of 4 words per pixel
 *   9. kf_set_model_maps_rays_color                -> model maps and KF_MAP_RAYCAST_RGB on every member
 * and kf_group_marching_cubes extracts with colour.
 * with near / far planes trunc_min / trunc_max.  No host synchronisation and no memset / memcpy of a per-frame buffer inside
 * kf_group_frame: the kernels write every pixel of their outputs.
 *
 * Backends:
 *   KF_GROUP_LOCAL      N members on ONE device, one group stream.  The two all-reduces are streaming kernels that reduce the N
 *                       members' buffers into one group buffer which every member then reads.  For checking the protocol and for
 *                       one-GPU use: it is NOT faster than one whole-volume context (every member marches every ray and runs its own ICP).
 *   KF_GROUP_RCCL_ALL   one process, one member per device (distinct devices), one communicator per member (ncclCommInitAll);
 *                       each member on its context's own stream, the N calls of a collective inside ncclGroupStart / End.
 *   KF_GROUP_RCCL_RANK  one process per GPU (torchrun / MPI style): one member here, ncclCommInitRank from a unique id that the
 *                       caller obtained on one rank with kf_group_unique_id and handed to every rank.
 *
 * Status codes are those of libhybkf.so (0 ok, hip errors, KF_GROUP_ERR_*); kf_group_error_string names them.  Every entry point
 * restores the caller's current HIP device.  A member call that fails mid-frame puts the group into a failed state: every later
 * call returns KF_GROUP_ERR_STATE (kf_group_destroy still frees it), and no collective is issued after the failure.
 */
#ifndef HYBKF_GROUP_H_
#define HYBKF_GROUP_H_
#include <stdint.h>
#include <stddef.h>
#include "hybkf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kf_group kf_group;

enum { KF_GROUP_LOCAL = 0, KF_GROUP_RCCL_ALL = 1, KF_GROUP_RCCL_RANK = 2 };
enum { KF_GROUP_MAX_MEMBERS = 16, KF_GROUP_UNIQUE_ID_BYTES = 128, KF_GROUP_MAX_TIMED_FRAMES = 4096 };
/* the same values as libhybkf.so's own argument / state / allocation errors; KF_GROUP_ERR_RCCL: an RCCL call failed */
enum { KF_GROUP_ERR_ARG = 1001, KF_GROUP_ERR_STATE = 1002, KF_GROUP_ERR_ALLOC = 1003, KF_GROUP_ERR_RCCL = 1004 };

/* what pipeline.SlabPipeline reads from scene.STOCK and its workload dict */
typedef struct kf_group_params {
  float trunc_min, trunc_max;           /* depth gate of kf_preprocess, also the raycast's near / far planes */
  float sigma_pixel, sigma_depth;       /* bilateral filter */
  kf_icp_params icp;                    /* pyramid_levels is taken from the base config */
  kf_integrate_params integrate;
  kf_raycast_params raycast;
} kf_group_params;

const char* kf_group_error_string(int status);

/* ncclGetUniqueId into out (KF_GROUP_UNIQUE_ID_BYTES bytes), for KF_GROUP_RCCL_RANK */
int kf_group_unique_id(uint8_t out[128]);

/* Checked before any HIP or RCCL call (KF_GROUP_ERR_ARG):
 *   members in 1..16; LOCAL / RCCL_ALL: the whole layout, z_cuts[0] = 0, z_cuts[members] = resolution, rising strictly, multiples of 8;
 *   RCCL_RANK: members = 1 and z_cuts = {z0, z1}, this rank's own slab: multiples of 8, z0 < z1 <= resolution, z0 = 0 exactly for rank 0
 *   and z1 = resolution exactly for rank world - 1 (every rank passes its own pair; the pairs of ranks 0 .. world-1 must tile the volume);
 *   halo (0: computed) not thinner than ceil(ray_increment / voxel) + 2 rounded up to 8 layers (pipeline.slab_halo_layers);
 *   base->has_color == 0 (colour: kf_group_create_color);
 *   devices (NULL: base->device for every member): LOCAL all equal, RCCL_ALL all distinct, RCCL_RANK exactly one member;
 *   unique_id / rank < world only for RCCL_RANK (ignored otherwise).
 * base->slab_* are ignored: each member's slab comes from z_cuts. */
int kf_group_create(const kf_config* base, const kf_group_params* params, int backend, uint32_t members, const uint32_t* z_cuts,
                    const int32_t* devices, uint32_t halo, const uint8_t* unique_id, uint32_t rank, uint32_t world, kf_group** out);
/* the same checks alone, without creating anything (no HIP or RCCL call): 0 or KF_GROUP_ERR_ARG */
int kf_group_validate(const kf_config* base, const kf_group_params* params, int backend, uint32_t members, const uint32_t* z_cuts,
                      const int32_t* devices, uint32_t halo, const uint8_t* unique_id, uint32_t rank, uint32_t world);
/* A COLOUR group: the arguments of kf_group_create / kf_group_validate plus the colour weighting switch of kf_integrate_volume.  The same checks, except:
 * base->has_color == 1 and a non-empty base->rgb_camera are REQUIRED (KF_GROUP_ERR_ARG otherwise).  kf_group_create / kf_group_validate keep refusing colour. */
int kf_group_create_color(const kf_config* base, const kf_group_params* params, int use_angle_weight_color, int backend, uint32_t members,
                          const uint32_t* z_cuts, const int32_t* devices, uint32_t halo, const uint8_t* unique_id, uint32_t rank, uint32_t world,
                          kf_group** out);
int kf_group_validate_color(const kf_config* base, const kf_group_params* params, int use_angle_weight_color, int backend, uint32_t members,
                            const uint32_t* z_cuts, const int32_t* devices, uint32_t halo, const uint8_t* unique_id, uint32_t rank, uint32_t world);
int kf_group_destroy(kf_group* g);
int kf_group_members(kf_group* g, uint32_t* members, uint32_t* halo);
/* every member's device-resident pose (kf_set_pose).  kf_group_create already sets HybKinectfu::init's: identity rotation, camera at
 * (size / 2, size / 2, -trunc_min) */
int kf_group_set_pose(kf_group* g, const kf_mat44* pose);

/* Enqueue one frame (asynchronous).  on_device = 0: mm is host memory, copied once per device; on_device = 1: mm is device memory
 * that every member's device can read (for one device: a plain device buffer).  It must stay unchanged until the frame's
 * preprocess has run on every member (kf_group_synchronize, or stream order on a caller stream that follows the group's). */
int kf_group_frame(kf_group* g, const uint16_t* mm, int on_device, uint32_t cols, uint32_t rows, uint32_t frame_id);
/* the same with one device frame per member (RCCL_ALL across devices: each member reads the copy on its own device) */
int kf_group_frame_members(kf_group* g, const uint16_t* const* dev_mm, uint32_t cols, uint32_t rows, uint32_t frame_id);
/* The frame calls of a colour group: the same with the frame's BGR image (3 bytes per pixel, base->rgb_camera's size), which lies where the depth frame
 * lies -- host memory copied once per device (on_device = 0), or device memory every member can read / one device image per member.  cols, rows are the
 * depth frame's.  A colour group refuses kf_group_frame / kf_group_frame_members and a colourless group refuses these two with KF_GROUP_ERR_STATE: nothing
 * is enqueued, no collective is issued, and the group stays usable. */
int kf_group_frame_color(kf_group* g, const uint16_t* mm, const uint8_t* bgr, int on_device, uint32_t cols, uint32_t rows, uint32_t frame_id);
int kf_group_frame_members_color(kf_group* g, const uint16_t* const* dev_mm, const uint8_t* const* dev_bgr, uint32_t cols, uint32_t rows, uint32_t frame_id);
/* member 0's kf_read_track_result (blocking).  check_lockstep: also compare every member's pose bits, verdict, status and
 * frames fused / lost with member 0's; a disagreement returns KF_GROUP_ERR_STATE (in-process members only: a RCCL_RANK
 * group compares nothing across processes). */
int kf_group_track_result(kf_group* g, kf_track_result* out, int check_lockstep);
/* borrowed: for read-backs (maps, volume, stats).  The group owns the context and its stream; do not destroy it or change its stream.
 * Viewer frames (hybkf.h): after step 9 every member holds the merged model maps, so kf_view_model_maps on any member -- member 0 by
 * convention -- gives the whole volume's picture from the tracking camera.  A FREE viewpoint over a group is kf_group_render_view below:
 * kf_render_view itself refuses a member that does not own the whole volume (KF_ERR_STATE), because it sees only its own layers. */
int kf_group_member(kf_group* g, uint32_t i, kf_ctx** out);
/* A merged view: the whole volume from any camera and pose, 4 display bytes per pixel (hybkf.h: KF_VIEW_*, the same bytes as kf_render_view on a
 * whole-volume context).  kf_group_render_view enqueues, on the members' streams (asynchronous):
 *   1. kf_view_slab_cross on every member   2. MIN all-reduce of the crossing words   3. kf_view_slab_normals on every member
 *   4. integer SUM all-reduce of the candidates   5. kf_view_from_rays on member 0 -- the first member this process holds
 * with the group's own ray increment (so the halo the group was created with suffices) and the caller's planes.  The candidates have 4 words per
 * pixel only for KF_VIEW_COLOR: the other two modes run the colourless forms on a colour group too.  pose NULL: the device-resident pose (the
 * same bits on every member); a given pose is used as it is by every member.  dev_v / dev_n: optional float4 maps of view_cam's size on member
 * 0's device (kf_view_from_rays).  KF_GROUP_RCCL_RANK: the call is collective -- every rank issues it with the same arguments, and only those
 * are checked.  The view's buffers are the group's own (a view never touches a frame's), grow on demand and are freed by kf_group_destroy.
 * It is a bystander to kf_group_frame*: poses, launch forms, kf_get_raycast_form's records, model maps and volumes are the same with and
 * without views between frames, and the merge timers do not count it.
 * kf_group_view_validate: the refusals, without any HIP call -- KF_GROUP_ERR_ARG for a mode outside KF_VIEW_* or a camera outside kf_render_view's
 * limits, KF_GROUP_ERR_STATE for KF_VIEW_COLOR with color_group == 0.  After such a refusal nothing is enqueued, no collective is issued and the
 * group stays usable; a member call or a collective that fails mid-sequence puts the group into the failed state, as in a frame.
 * kf_group_view_size / kf_group_view_device / kf_group_read_view (blocking): member 0's kf_view_size / kf_view_device / kf_read_view after a
 * merged view; KF_GROUP_ERR_STATE (NULL) before one. */
int kf_group_view_validate(int color_group, int mode, const kf_camera_params* view_cam);
int kf_group_render_view(kf_group* g, int mode, const kf_mat44* pose, const kf_camera_params* view_cam, float near_plane, float far_plane,
                         float* dev_v, float* dev_n);
int kf_group_view_size(kf_group* g, uint32_t* cols, uint32_t* rows);
const uint8_t* kf_group_view_device(kf_group* g);
int kf_group_read_view(kf_group* g, uint8_t* dst, size_t dst_bytes);
/* kf_marching_cubes on every member (each extracts its own layers); a colour group extracts with colour */
int kf_group_marching_cubes(kf_group* g, float threshold);
int kf_group_triangle_count(kf_group* g, uint32_t* count);                                     /* sum over the members, blocking */
/* triangles [first, first + count) of the slab-major sequence: member 0's, then member 1's, ... = the whole volume's canonical order */
int kf_group_read_triangles(kf_group* g, kf_triangle* dst, uint32_t first, uint32_t count);
/* hipEvent pair around each frame's merge (steps 6-9), on member 0's stream; kf_group_read_merge_ms blocks, returns the total
 * and the frame count since the last read, and resets them.  At most KF_GROUP_MAX_TIMED_FRAMES frames are timed between two reads
 * (the event pool stops growing there; later frames run untimed and are not counted): read at least that often. */
int kf_group_merge_timing(kf_group* g, int on);
int kf_group_read_merge_ms(kf_group* g, float* total_ms, uint32_t* frames);
int kf_group_synchronize(kf_group* g);

/* The moving volume over a group (hybkf.h: kf_shift_volume, and kf_shift_slab for THE RULE and the transit layout).  A group shifts its window by whole
 * bricks on any axis, in place and on the members' streams; every member's stored layers -- owned and halo -- end up bit for bit what a whole-volume
 * context holds there after kf_shift_volume.  An x or y shift is local to every member; a z shift moves brick layers between members.
 * kf_group_shift_plan: the transfers of a z shift by dz voxels, host only (no HIP or RCCL call) -- the one place the rule "who feeds whom" lives, and what
 *   kf_group_shift_volume executes.  For every member (stored brick layers: its slab of z_cuts plus `halo` voxel layers on each side, rounded up to
 *   bricks, clamped to the volume) it takes the need range -- the source layers p + dz / 8 of its stored layers p that lie inside the volume and are not
 *   stored there (kf_slab_shift_needs) -- and cuts it by who OWNS each layer: the member j whose [z_cuts[j], z_cuts[j + 1]) holds it.  Layers nobody has
 *   to send (they lie outside the volume) read as never observed.  Order: by receiver, then by layer.  Writes at most `cap` transfers and returns their
 *   number (call again with a larger buffer if it exceeds cap), or -1 for bad arguments: a resolution that is no multiple of 8, cuts that do not tile
 *   [0, resolution) rising in multiples of 8, a dz that is no multiple of 8, out NULL with cap > 0.
 * kf_group_shift_volume: asynchronous on the members' streams, three steps --
 *   1. every owner packs what the plan sends (kf_slab_pack_layers): LOCAL straight into the receiver's feed buffer at the layer's offset, RCCL into a
 *      send buffer;   2. the exchange: LOCAL needs none (one stream: every pack precedes every move), RCCL_ALL / RCCL_RANK ncclSend / ncclRecv of bytes
 *      inside one ncclGroupStart / End on the members' streams;   3. kf_shift_slab on every member with its feed.
 *   Every pack of the whole group precedes every move: an owner's layers leave before it overwrites them.  Feed and send buffers are the group's own,
 *   sized to the plan (not to the slab), grow on demand (only then does the call block) and are freed by kf_group_destroy.  The cuts do not change
 *   (re-balancing stays kf_resize_slab's job); brick store, stream-out and map mesh stay whole-volume features: a group's window forgets what leaves.
 *   KF_GROUP_RCCL_RANK: the call is collective; the first shift all-gathers the ranks' (z0, z1) once (blocking) and keeps them, so every rank derives
 *   the same plan.  d = (0, 0, 0) returns 0 and enqueues nothing.  KF_GROUP_ERR_ARG, with nothing enqueued, no collective issued and the group still
 *   usable: a component that is no multiple of 8, a sum of shifts beyond 32 bits.  A failure mid-sequence puts the group into the failed state.
 *   THE MODEL MAPS ARE STALE on every member afterwards: call kf_group_raycast before the next frame.
 * kf_group_raycast: steps 5-9 of kf_group_frame alone -- the merged raycast from the device-resident pose, in the colour forms on a colour group;
 *   the whole-volume counterpart is kf_raycast_volume(transform = NULL).  Asynchronous; collective on RCCL_RANK.
 * kf_group_volume_origin: member 0's kf_volume_origin; in-process members that disagree give KF_GROUP_ERR_STATE. */
typedef struct kf_group_transfer { uint32_t from_member, to_member, bz_begin, bz_end; } kf_group_transfer;   /* brick layers [bz_begin, bz_end) */
int kf_group_shift_plan(uint32_t resolution, uint32_t members, const uint32_t* z_cuts, uint32_t halo, int32_t dz, kf_group_transfer* out, uint32_t cap);
int kf_group_shift_volume(kf_group* g, int32_t dx, int32_t dy, int32_t dz);
int kf_group_raycast(kf_group* g);
int kf_group_volume_origin(kf_group* g, int32_t origin_vox[3]);
/* the stream member i's work is enqueued on (LOCAL: the one group stream) */
void* kf_group_stream(kf_group* g, uint32_t i);

#ifdef __cplusplus
}
#endif
#endif /* HYBKF_GROUP_H_ */
