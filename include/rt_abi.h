/*
 * rt_abi.h — C ABI of the MI355X-native path tracer (librtamd.so).
 *
 * Drop-in boundary for isaac-chandler/cuda-raytracer's GPU render path.  Plain C types,
 * pointers and sizes only; no HIP or torch types cross this boundary.  Every entry point
 * names the reference interface it replaces (file:line in the reference checkout).
 *
 * Byte layouts of the scene arrays are the reference's (scene.cuh:9-100):
 *   rt_sphere 16 B, rt_triangle 48 B (ray-tracing representation: p1, p2-p1, p3-p1,
 *   normalise(cross(p3-p1, p2-p1))), rt_material 48 B, rt_bvh_node 32 B,
 *   uint16 material indices (spheres first, then triangles), env map float[h][w][3].
 *
 * Errors: every int-returning call returns 0 on success or a negative RT_E_* code and
 * records a message readable with rt_last_error() (thread-local).  The reference printed
 * "Error <expr> <msg>" and exit(1) instead (common.cuh:10-18); the CLI keeps that.
 * Hardware queues: loading the library sets GPU_MAX_HW_QUEUES=24 unless the host has set it (HIP
 * reads it at initialisation; 4 by default), and a renderer keeps at most that many passes in flight,
 * one stream each (up to 20).
 * Threading: calls are blocking.  One rt_renderer is bound to one device and must not be
 * used from two threads at once; distinct renderers may run concurrently.
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 7

enum {
    RT_OK = 0,
    RT_E_INVALID = -1,   /* bad argument / scene */
    RT_E_IO = -2,        /* file could not be read or written */
    RT_E_HIP = -3,       /* HIP runtime error (message has the HIP error string) */
    RT_E_NODEVICE = -4,  /* no HIP device / HIP kernels not loadable */
    RT_E_OOM = -5        /* device allocation failed */
};

typedef struct { float x, y, z; } rt_vec3;
typedef struct { rt_vec3 center; float radius; } rt_sphere;                          /* scene.cuh:9  */
typedef struct { rt_vec3 p1, p2p1, p3p1, normal; } rt_triangle;                      /* scene.cuh:27 */
typedef struct {                                                                      /* scene.cuh:42 */
    rt_vec3 diffuse_albedo; float metallicity;
    rt_vec3 specular_albedo; float roughness;
    rt_vec3 emitted; float index_of_refraction;
} rt_material;
typedef struct { rt_vec3 min_bound, max_bound; int32_t child1, child2; } rt_bvh_node; /* scene.cuh:82 */

/* Host view of a loaded scene; mirrors `struct Scene` (scene.cuh:102-152). All pointers are
 * borrowed host memory.  environment_map holds width * height texels and must be at least as wide as
 * tall: the sky lookup's row stride is the map's height (scene.cu:389-391), which stays inside the map
 * only then; every call that renders an rt_scene or makes it resident refuses a taller map with
 * RT_E_INVALID, as does rt_scene_load. */
typedef struct {
    const rt_sphere *spheres;         int32_t sphere_count;
    const rt_triangle *triangles;     int32_t triangle_count;
    const uint16_t *material_indices;
    const rt_material *materials;     int32_t material_count;
    const rt_bvh_node *bvh;           int32_t bvh_node_count;
    int32_t width, height;
    const rt_vec3 *environment_map;   int32_t environment_map_width, environment_map_height;
    rt_vec3 camera_position, forward, up;
    float vertical_fov, exposure;
    rt_vec3 min_coord, inv_dimensions;
    rt_vec3 scaled_right, scaled_up, near_plane_top_left;
    float inv_width, inv_height;
    int32_t bounces, ray_count;
} rt_scene;

/* ------------------------------------------------------------------ scene loading (host)
 * Replaces load_scene(Scene*, const char*, bool use_bvh) (scene.cu:569-831) including
 * load_ply (:491), load_pfm (:548), precompute_camera_data (:62) and the binned-SAH
 * generate_bvh (:1002-1036).  CRLF scene files are accepted (the reference read them in
 * Windows text mode).  Prints the reference's stdout lines unless opts->quiet. */
typedef struct {
    int32_t use_bvh;          /* 1 = BVH depth 30 (default); 0 = `no_bvh` (single leaf)      */
    int32_t quiet;            /* 1 = suppress "Triangle count"/"BVH Took"/... stdout lines      */
    const char *asset_root;   /* directory relative asset paths resolve against; NULL = CWD  */
    int32_t image_override;   /* 1 = replace the scene's `image` W H spp bounces with below   */
    int32_t width, height, ray_count, bounces;
    int32_t exposure_override;
    float exposure;
    int32_t bvh_device;       /* -1 = build the BVH on the host (default); >= 0 = on that HIP device
                                 (same node array, triangle and material-index order)          */
} rt_load_opts;

typedef struct rt_scene_host rt_scene_host;   /* owns the arrays a rt_scene points into */

/* Refuses (RT_E_INVALID, the message names the primitive; before either BVH builder runs) a triangle or
 * sphere with a NaN or infinite coordinate or radius, and a triangle whose vertex sum overflows (a
 * non-finite centroid): the reference's bin index (scene.cu:916) is undefined for them. */
int rt_scene_load(const char *path, const rt_load_opts *opts, rt_scene_host **out);
const rt_scene *rt_scene_view(const rt_scene_host *scene);
double rt_scene_bvh_ms(const rt_scene_host *scene);          /* "BVH Took" (scene.cu:1026) */
void rt_scene_free(rt_scene_host *scene);

/* ------------------------------------------------------------------ GPU render
 * Pass p (0-based) of a render casts rtc = min(spp - 20p, 20) rays per pixel with
 * generate-seed `remaining` = spp - 20p - rtc (raytracing.cu:222-229). */
typedef struct {
    int32_t sort;         /* 1 = ray reordering after each bounce but the last (default);
                             0 = `no_sort` (raytracing.cu:238)                             */
    int32_t device;       /* HIP device ordinal                                          */
    int32_t pass_begin;   /* first pass to render (0)                                    */
    int32_t pass_count;   /* passes to render; -1 = all remaining                        */
    int32_t pass_stride;  /* render passes pass_begin, +stride, ... (multi-GPU pass shard) */
    int32_t collect_counters; /* 1 = also count traversal work (Pn/Iv/Tt) for the byte model */
    /* Pixel-tile sharding: the image is cut into stripes of tile_rows rows, dealt
     * round-robin to tile_count owners; this render casts only the rays of owner tile_index's
     * stripes, with their global ray indices (so seeds are the 1-GPU ones), and leaves the other
     * pixels 0.  With sort = 1 the process seeds follow the global post-sort slot
     * (raytracing.cu:89, :238-247), which needs the per-bounce exchange of
     * rt_renderer_set_exchange.  tile_count 0 or 1 = the whole image (default). */
    int32_t tile_count;
    int32_t tile_index;
    int32_t tile_rows;    /* stripe height in rows; 0 = 8 */
    /* Multi-GPU in one process (rt_render only): device_count > 1 renders whole
     * passes round-robin over device_ids[0..device_count) (NULL = devices 0..device_count-1), one
     * host thread and renderer per device, in one RCCL communicator (ncclCommInitAll).  Pass
     * framebuffers are exchanged as pixel slices (ncclAllToAll over xGMI: slice j goes to device
     * j, which adds the slices in pass order, bit-identical to one device) and the finished
     * slices are gathered to device_ids[0] (ncclGather), then copied to fb_out.  0 or 1 = the
     * single device `device`.  The reference ran one device (raytracing.cu:170-284). */
    int32_t device_count;
    const int32_t *device_ids;
    /* With device_count >= 1: 0 = pass sharding (above, the default); 1 = pixel tiles: device k
     * renders owner k's tile_rows-row stripes of every pass, with sort on through the
     * per-bounce bucket-byte ncclAllReduce (rt_renderer_set_exchange), and an ncclReduce of the
     * owners' framebuffers (disjoint pixels, the rest 0) to device_ids[0]. */
    int32_t shard_tiles;
} rt_opts;

typedef struct {
    uint64_t generated_rays;   /* rays generated (sum of n over passes)                    */
    uint64_t live_segments;    /* process_ray invocations on live slots                    */
    uint64_t sorted_items;     /* slots moved by the reorder                               */
    uint64_t nodes_popped;     /* Pn, only with collect_counters                           */
    uint64_t internal_visits;  /* Iv, only with collect_counters                           */
    uint64_t triangle_tests;   /* Tt, only with collect_counters                           */
    uint64_t sphere_tests;     /* S x live segments                                        */
    uint64_t hits, misses;     /* closest-hit outcomes over live segments                  */
    uint64_t hits_sphere;      /* subset of hits on spheres (the rest hit triangles)       */
    uint64_t dead_slots;       /* slots skipped by the terminated-key early-out            */
    uint32_t passes, reserved;
    double render_ms;          /* host wall time of the call (the "GPU Took" span)         */
    double kernel_ms;          /* HIP-event time of the whole pass loop on the stream      */
    double process_ms;         /* HIP-event time summed over the process (traversal) launches */
    double sort_ms;            /* HIP-event time summed over the reorder launches          */
    double trace_ms;           /* trace_kernel launches, summed: each launch's span on the device
                                  wall clock from its first wave's start to its last wave's end
                                  (event timing on; 0 for scenes without triangles, which have
                                  no trace launch)                                          */
    uint64_t trace_launches;   /* trace_kernel launches timed in trace_ms                  */
    /* rt_render runs without per-bounce events (like the benchmark's timed passes): its process_ms,
       sort_ms and trace_ms stay 0 unless RTAMD_EVENTS=1; rt_renderer_run has them by default */
    double exchange_ms;        /* multi-GPU rt_render: host wall time of the RCCL slice exchange
                                  and gather (max over devices).  The multi-GPU render runs
                                  without per-bounce events: process_ms, sort_ms and trace_ms
                                  stay 0 there unless RTAMD_MULTI_EVENTS=1                  */
} rt_stats;

void rt_default_opts(rt_opts *opts);
void rt_default_load_opts(rt_load_opts *opts);
int rt_device_count(void);
/* Initialises the HIP runtime, the device's queues and the kernel code object on `device`
 * (what the first render would otherwise pay, ~0.2 s per process).  Thread-safe; a host can call
 * it on a thread of its own while it loads the scene, as the CLI does.  No reference
 * counterpart: the reference pays CUDA context creation inside gpu_raytrace (raytracing.cu:174). */
int rt_device_warmup(int32_t device);

/* Replaces `Vec3 *gpu_raytrace(const Scene *scene, bool sort)` (raytracing.cu:170-284):
 * uploads the scene, renders every pass selected by opts, and writes the accumulated
 * framebuffer (W*H*3 floats, raw radiance sums, caller-owned) to fb_out. */
int rt_render(const rt_scene *scene, const rt_opts *opts, float *fb_out, rt_stats *stats);

/* Persistent renderer: scene resident in HBM, ray buffers sized for 20 rays/pixel per pass,
 * up to 20 passes in flight on separate streams (each with its own buffer set) so one pass's
 * latency-bound last bounces overlap another's throughput-bound first bounces.  The framebuffer
 * adds stay in pass order.  Used by rt_render, the benchmark and the multi-GPU drivers. */
typedef struct rt_renderer rt_renderer;
int rt_renderer_create(const rt_scene *scene, const rt_opts *opts, rt_renderer **out);
/* Renders passes pass_begin, pass_begin+stride, ... (count passes) and adds each pass's
 * per-pixel sum into the renderer's device framebuffer (ordered: fb += pass_sum, pass
 * order).  If d_pass_sums != NULL (device pointer, count*W*H*3 floats) the pass sums are
 * also stored there.  Blocking. */
int rt_renderer_run(rt_renderer *r, int32_t pass_begin, int32_t count, int32_t stride,
                    float *d_pass_sums, rt_stats *stats);
/* The same passes enqueued without waiting (d_pass_sums required, not for pixel tiles with sort
 * on): rt_renderer_wait_pass makes a caller's HIP stream (a hipStream_t on r's device) wait until
 * the k-th pass of the run (0-based) has written its sums, so the caller can exchange finished
 * passes while later ones render (the multi-GPU slice exchange); rt_renderer_finish waits for the
 * whole run and fills stats.  The framebuffer adds and every other rule are those of
 * rt_renderer_run.  Until rt_renderer_finish returns, every other call on r that runs passes,
 * touches the framebuffer or changes the run's settings (run, run_host, read/copy_framebuffer,
 * clear, set_event_timing, set_counters, launch_profile) fails with RT_E_INVALID and changes
 * nothing.  No reference counterpart (the reference's gpu_raytrace returned at the end). */
int rt_renderer_run_async(rt_renderer *r, int32_t pass_begin, int32_t count, int32_t stride, float *d_pass_sums);
int rt_renderer_wait_pass(rt_renderer *r, int32_t k, void *hip_stream);
int rt_renderer_finish(rt_renderer *r, rt_stats *stats);
/* Same, with the per-pass sums returned in host memory (count*W*H*3 floats). */
int rt_renderer_run_host(rt_renderer *r, int32_t pass_begin, int32_t count, int32_t stride,
                         float *host_pass_sums, rt_stats *stats);
int rt_renderer_read_framebuffer(rt_renderer *r, float *fb_out);   /* device fb -> host     */
int rt_renderer_copy_framebuffer(rt_renderer *r, float *d_out);    /* device fb -> device ptr on
                                                                       r's device (W*H*3 floats) */
int rt_renderer_clear(rt_renderer *r);                               /* zero the device fb    */
/* Pixel tiles with the reorder on (tile_count > 1, sort = 1).  The process seed is the
 * ray's GLOBAL post-sort slot (raytracing.cu:89 after :238-247), so after every bounce but the
 * last the owners exchange one byte per global live ray: each writes bucket + 1 at the global slot
 * of each of its live rays into a zeroed array of n bytes, and `exchange` must sum the arrays of
 * all owners in place (an all-reduce: every slot has one owner, no byte exceeds 65) and return 0.
 * Each owner then ranks its rays as the stable sort of all keys would; rays never migrate.
 * on_device = 1: `bytes` is a device pointer on the renderer's device and the exchange is enqueued
 * on (or completed before returning from) `hip_stream`, a hipStream_t; 0: `bytes` is host memory
 * and the exchange completes before returning.  Calls come in the same order on every owner
 * (pass by pass of a group in flight, bounce by bounce).  Without an exchange such a render fails. */
typedef int (*rt_exchange_fn)(void *user, uint8_t *bytes, uint64_t n, void *hip_stream);
int rt_renderer_set_exchange(rt_renderer *r, rt_exchange_fn fn, void *user, int32_t on_device);
/* The same exchange over RCCL for one process per GPU (torchrun-style hosts): the renderer joins
 * an RCCL communicator of nranks owners (ncclCommInitRank; blocks until every rank has joined) and
 * sums the bytes with an in-place ncclAllReduce(uint8) on the pass's stream, so no byte leaves
 * the device.  Every rank passes the same RT_RCCL_ID_BYTES-byte id: rank 0 makes it with
 * rt_rccl_unique_id and the host hands it to the others (e.g. a torch.distributed broadcast).
 * The communicator is the renderer's and is destroyed with it.  No reference counterpart: the
 * reference ran one device (raytracing.cu:170-284). */
#define RT_RCCL_ID_BYTES 128
int rt_rccl_unique_id(uint8_t *id_out);
int rt_renderer_set_exchange_rccl(rt_renderer *r, const uint8_t *id, int32_t nranks, int32_t rank);
int rt_renderer_set_counters(rt_renderer *r, int32_t enable);
/* Framebuffer accumulation (default on).  Off, a run must be given d_pass_sums and only writes them:
 * no pass is added into the renderer's framebuffer, so no pass's stream waits for another's (the
 * in-order add chain is what the multi-GPU drivers, which add the pass slices themselves, turn off).
 * No reference counterpart. */
int rt_renderer_set_accumulate(rt_renderer *r, int32_t enable);
/* Per-bounce HIP events behind rt_stats.process_ms / sort_ms (default on).  Off, those stay 0 and
 * a pass's stream carries no marker packets between its kernels (~2 % faster frames). */
int rt_renderer_set_event_timing(rt_renderer *r, int32_t enable);
/* Per trace launch of the last run's first pass (event timing on): trace_ms_out[b] = the launch's
 * device wall-clock span (first wave start to last wave end) and live_out[b] = the live rays it
 * traced, for bounce b < cap.  Returns the number of launches written (0 without event timing or
 * for scenes without triangles).  Live counts are known only for runs of at most as many passes
 * as are in flight (the benchmark's one-pass exclusive run); in a longer run live_out[b] is 0.
 * Measurement only; no reference counterpart. */
int rt_renderer_launch_profile(rt_renderer *r, int32_t cap, double *trace_ms_out, uint32_t *live_out);
void rt_renderer_destroy(rt_renderer *r);

/* Persistent multi-GPU renderer (one process): rt_render's device_count >= 1 pass sharding
 * with its set-up kept between renders -- one RCCL communicator over device_ids[0..device_count)
 * (ncclCommInitAll; NULL = devices 0..device_count-1), one renderer per device (scene resident, 16
 * passes in flight each) and the slice-exchange buffers.  opts as for rt_render (sort,
 * collect_counters, device_count, device_ids; pass sharding only: shard_tiles and tile_count are
 * refused).  rt_multi_create fails with RT_E_NODEVICE when a listed device does not exist, and checks
 * that every communicator rank answers (an all-reduce of one int per device; rt_multi_ranks returns the
 * count).  rt_multi_run renders passes 0..pass_count-1 of the frame (-1 = all) round-robin over the
 * devices (pass p on device p mod N), exchanges the pass sums as pixel slices while later passes
 * render (ncclAllToAll; each owner adds its slice in pass order, so the image is bit-identical to one
 * device's) and gathers the frame on device_ids[0]; fb_out (host, W*H*3 floats) receives it unless
 * NULL, and rt_multi_read_framebuffer copies the last run's frame later.  A run that fails after its
 * devices started leaves the object unusable (its communicators may be aborted): destroy it.
 * Blocking; one call at a time per object.  No reference counterpart: the reference ran one device
 * and allocated per call (raytracing.cu:170-284). */
typedef struct rt_multi rt_multi;
int rt_multi_create(const rt_scene *scene, const rt_opts *opts, rt_multi **out);
int rt_multi_run(rt_multi *m, int32_t pass_count, float *fb_out, rt_stats *stats);
int rt_multi_read_framebuffer(rt_multi *m, float *fb_out);
int rt_multi_set_event_timing(rt_multi *m, int32_t enable);   /* per-bounce events (default off) */
int rt_multi_set_counters(rt_multi *m, int32_t enable);       /* traversal counters (Pn/Iv/Tt)   */
int rt_multi_ranks(const rt_multi *m);
void rt_multi_destroy(rt_multi *m);

/* Closest hit of n caller rays: rays = n x {o.x o.y o.z d.x d.y d.z} (d unit length, as every
 * ray the render traces).  The sphere loop (scene.cu:338-372) then bvh_closest_hit_distance
 * (scene.cu:134-241) -- one bounce of process_ray up to the hit (scene.cu:320-374) -- through
 * the render's traversal kernel.  t_out[i] = closest distance (1e30 when nothing is hit),
 * index_out[i] = primitive index (spheres first, then sphere_count + triangle; -1 = miss).
 * With opts->collect_counters the traversal counters are returned in stats.  One call is
 * rt_query_create + rt_query_closest_host + rt_query_destroy; t_out, index_out and stats may be NULL. */
int rt_trace_rays(const rt_scene *scene, const rt_opts *opts, const float *rays, int32_t n,
                  float *t_out, int32_t *index_out, rt_stats *stats);

/* Resident ray queries: the scene and BVH stay in HBM (the object costs the scene plus its scratch: no
 * framebuffer, no pass contexts) and device pointers go in and out on the caller's stream.
 * The presence of these symbols is the feature probe; RT_ABI_VERSION, rt_opts and rt_stats are unchanged.
 * No reference counterpart as an interface (the reference traced only its own render's rays); what each
 * call computes restates the reference's traversal:
 *   rt_query_closest   the sphere loop (scene.cu:338-372) then bvh_closest_hit_distance (scene.cu:134-241)
 *                      with `closest` starting at 1e30 -- rt_trace_rays' semantics exactly (t = 1e30 and
 *                      index = -1 on a miss, NaN behaviour included), through the render's trace kernel.
 *   rt_query_occluded  the same sphere loop and traversal with `closest` held at the ray's bound B and
 *                      never updated: 1 iff some primitive is accepted.  B = tmax[i] where tmax[i] <= 1e30,
 *                      otherwise (larger, +inf, NaN, or d_tmax NULL) 1e30.  That is: every sphere tested
 *                      with closest = B (scene.cu:340-371); the root entered iff !(0 >= B); in a leaf every
 *                      triangle tested with closest = B (scene.cu:160-195); at an internal node a child
 *                      entered iff ray_aabb_intersection(child, tmax = B) (scene.cu:109-132) holds and
 *                      !(entry >= B) (scene.cu:147-152).  t < 0.005 rejects as everywhere.  Because B never
 *                      shrinks, which nodes are entered does not depend on the visit order, so the kernel
 *                      visits the near child first and stops at the first accepted primitive; the answer is
 *                      the reference-order answer bit for bit.  Against the closest hit (t_c, index):
 *                      occluded implies t_c < B, and for B = 1e30 occluded <=> index >= 0; t_c < B does NOT
 *                      imply occluded when B lies just above t_c (a box's float entry distance can exceed
 *                      the triangle's float t, and the fixed bound then prunes the box).
 * rays = n x {o.x o.y o.z d.x d.y d.z} floats, contiguous, d unit length.  The device-pointer calls take
 * pointers on q's device and enqueue on hip_stream (a hipStream_t, passed to HIP as given: NULL is HIP's
 * default stream, which is also torch's default); once the scratch holds n rays (rt_query_reserve, or an
 * earlier call of at least that size; it grows geometrically) they allocate nothing and never wait on the
 * host.  Each call records an event the next call's stream waits for, so alternating streams is safe; the
 * caller keeps its own buffers alive and unmodified until the call's work on hip_stream has finished.
 * The _host calls take host pointers and block.  n == 0 returns RT_OK and touches no pointer; a null
 * object, n < 0 or a null pointer with n > 0 (d_tmax / tmax excepted) return RT_E_INVALID before any HIP
 * call.  Uses opts->device and opts->collect_counters.  One thread at a time per object; distinct objects
 * may run concurrently.
 * rt_query_stats waits for the last call and returns its counters: live_segments = n, hits = the hit or
 * occluded count, misses = the rest, hits_sphere (closest only); with collect_counters also Pn/Iv/Tt and
 * sphere_tests -- the oracle's for closest; for occluded exact on unoccluded rays and order-dependent on
 * occluded ones (the sphere loop stops at the first accepted sphere). */
typedef struct rt_query rt_query;
int rt_query_create(const rt_scene *scene, const rt_opts *opts, rt_query **out);
int rt_query_reserve(rt_query *q, int32_t n);   /* size the scratch for n rays now */
int rt_query_closest(rt_query *q, const float *d_rays, int32_t n, float *d_t, int32_t *d_index, void *hip_stream);
int rt_query_occluded(rt_query *q, const float *d_rays, const float *d_tmax /* NULL = 1e30 */, int32_t n,
                      uint8_t *d_occluded /* 0 or 1 */, void *hip_stream);
int rt_query_closest_host(rt_query *q, const float *rays, int32_t n, float *t, int32_t *index);
int rt_query_occluded_host(rt_query *q, const float *rays, const float *tmax, int32_t n, uint8_t *occluded);
int rt_query_stats(rt_query *q, rt_stats *stats);
void rt_query_destroy(rt_query *q);

/* Dynamic geometry: new triangle vertices under the frozen BVH topology (a refit).  The
 * presence of these symbols is the feature probe; RT_ABI_VERSION and every struct are unchanged.  No
 * reference counterpart (the reference's scenes are static).
 * vertices = triangle_count x 9 floats, {a.xyz, b.xyz, c.xyz} per triangle IN THE SCENE'S TRIANGLE ORDER
 * (rt_scene.triangles, i.e. after the builder's permutation); triangle_count must equal the scene's.
 *   triangle record i:  p1 = a, p2p1 = b - a, p3p1 = c - a, normal = normalise(cross(p3p1, p2p1)) with the
 *                       loader's normalise (scale(1 / sqrtf(dot), v)), no contraction.
 *   bounds:             from the absolute vertices, never from p1 + edge, with the loader's min/max
 *                       ((b < a) ? b : a, which keeps the earlier operand of a tie; never the hardware min,
 *                       which orders -0 below +0).  box(tri) = grow over a, b, c from (1e30, -1e30); a leaf
 *                       over [child2, child1) = grow over box(tri) in index order from (1e30, -1e30); an
 *                       internal node = grow(grow(init, box(child1)), box(child2)).  "Earliest of the
 *                       smallest" is associative, so this hierarchical fold is the builder's linear fold
 *                       over the node's range in the scene's triangle order.
 *   untouched:          child indices, leaf ranges, triangle order, material indices, spheres.
 * rt_scene_refit rewrites a loaded scene's triangles and node bounds in place (the rt_scene view stays
 * valid) and recomputes min_coord / inv_dimensions as the loader does; a render or query created from the
 * scene afterwards sees the new geometry, objects created earlier keep their own device copies.
 * rt_query_update_triangles does the same to q's resident records, bit-identical to rt_scene_refit, from
 * a device pointer on q's device: enqueued on hip_stream (one triangle kernel, then one launch per BVH
 * level from the deepest up, the levels that fit one workgroup chained in a single-workgroup launch; a
 * scene whose root is a leaf has no node records and gets the triangle kernel plus a one-workgroup fold of
 * the root's box, which only rt_query_read_geometry reads).  It allocates nothing and never waits on the
 * host.  It joins the queries' event chain: hip_stream first waits for the last call on q, and queries
 * enqueued later (on any stream) see the new geometry, earlier ones the old; d_vertices is read in stream
 * order and must stay alive and unmodified until then.  The _host variant stages host vertices (its
 * staging buffer is allocated by the first such call) and blocks.  After an update, with no query since,
 * rt_query_stats returns zeros.
 * rt_query_read_geometry waits for the last call, then copies out the device's current triangle records
 * (triangle_count) and/or the node array in the scene's numbering (bvh_node_count; the root's own box is
 * the merge of its two children's); either pointer may be NULL.  For inspection and tests.
 * Errors (RT_E_INVALID with a message, before any launch): a null object or pointer, triangle_count other
 * than the scene's.  triangle_count 0 on a scene without triangles is a no-op. */
int rt_scene_refit(rt_scene_host *scene, const float *vertices, int32_t triangle_count);
int rt_query_update_triangles(rt_query *q, const float *d_vertices, int32_t triangle_count, void *hip_stream);
int rt_query_update_triangles_host(rt_query *q, const float *vertices, int32_t triangle_count);
int rt_query_read_geometry(rt_query *q, rt_triangle *triangles_out, rt_bvh_node *bvh_out);

/* Hit records: the closest hit with what a caller needs of the surface.  The presence of these
 * symbols is the feature probe; RT_ABI_VERSION and every existing struct are unchanged.  No reference
 * counterpart as an interface; every field restates what the reference forms at the hit (scene.cu:160-195,
 * :398-418).
 * For ray i with origin o and direction d let (t, index) be exactly what rt_query_closest returns and S the
 * scene's sphere count.  All arithmetic is float32, each operation rounded once, no contraction;
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z,
 * a.x*b.y - a.y*b.x).
 *   t, index     unchanged (1e30 and -1 on a miss).
 *   miss         (index < 0): uv = (+0, +0), normal = position = (+0, +0, +0), material = -1, front_face = 0.
 *   position     o + t * d per component, a multiply then an add (scene.cu:398).
 *   triangle     record k = index - S (p1, e1 = p2p1, e2 = p3p1, normal):
 *                  h = cross(d, e2); a = dot(h, e1); f = 1 / a; s = o - p1;
 *                  u = dot(s, h) * f; q = cross(s, e1); v = dot(d, q) * f          (scene.cu:166-183)
 *                uv = (u, v): the hit lies at p1 + u e1 + v e2.  normal = the record's, unflipped
 *                (scene.cu:409-410).
 *   sphere       uv = (+0, +0); normal = (1 / radius) * (position - center) (scene.cu:405).
 *   front_face   dot(normal, d) < 0 (scene.cu:418).  The normal is returned unflipped: the reference's shading
 *                normal is its negation where front_face == 0.
 *   material     material_indices[index] as int32 (scene.cu:413).
 * The geometry is the object's current resident geometry: after rt_query_update_triangles the records come
 * from the refitted triangles (a zero-area triangle has a NaN normal and a = 0).  A NaN is any NaN: the sign
 * and payload of a NaN an operation produced are the processor's.
 * rt_hit_out: one output array per field, every pointer optional (NULL = not written); an rt_hit_out whose
 * fields are all NULL is allowed, the call then only traverses and counts.
 * rt_query_closest_hit follows every rule of rt_query_closest (device pointers on q's device, enqueued on
 * hip_stream, joins the event chain, allocates nothing once the scratch holds n rays, never waits on the
 * host; n == 0 is RT_OK and touches no pointer; a null object, n < 0, or a null d_rays or d_out with n > 0
 * is RT_E_INVALID before any HIP call).  d_out is a host pointer to a struct of device pointers, read
 * before the call returns.  rt_query_stats after it returns what it returns after rt_query_closest on the
 * same rays.  The _host variant takes host pointers throughout, stages through buffers of the object and
 * blocks.
 * rt_scene_hit_records is the host twin: the records of given (t, index) on a host scene, no GPU, bit for
 * bit what the device call writes for the same (t, index); out->t and out->index are ignored.  An index that
 * is not below sphere_count + triangle_count is RT_E_INVALID and nothing is written. */
typedef struct {            /* every pointer optional: NULL = not written */
    float   *t;             /* n        */
    int32_t *index;         /* n        */
    float   *uv;            /* n x 2    */
    float   *normal;        /* n x 3    */
    float   *position;      /* n x 3    */
    int32_t *material;      /* n        */
    uint8_t *front_face;    /* n, 0 / 1 */
} rt_hit_out;
int rt_query_closest_hit(rt_query *q, const float *d_rays, int32_t n, const rt_hit_out *d_out, void *hip_stream);
int rt_query_closest_hit_host(rt_query *q, const float *rays, int32_t n, const rt_hit_out *out);
int rt_scene_hit_records(const rt_scene *scene, const float *rays, const float *t, const int32_t *index,
                         int32_t n, const rt_hit_out *out);

/* Multi-hit queries: the K nearest hits of a ray, in order, and how many surfaces it crosses.  The
 * presence of these symbols is the feature probe; RT_ABI_VERSION and every existing struct are unchanged.  No
 * reference counterpart as an interface; every predicate restates the reference's traversal.
 * For ray i the bound B is rt_query_occluded's: B = tmax[i] where tmax[i] <= 1e30, otherwise (larger, +inf, NaN,
 * or a NULL tmax) 1e30.  H is the set of primitives the reference traversal accepts with `closest` held at B and
 * never updated:
 *   spheres      every sphere k is tested with closest = B (scene.cu:340-371); an accepted one contributes the
 *                hit (the t that test returns, k).
 *   root         entered iff !(0 >= B) (scene.cu:147-152).
 *   leaf         in an entered leaf every triangle j of [child2, child1) is tested with closest = B
 *                (scene.cu:160-195); an accepted one contributes (its t, sphere_count + j).
 *   internal     a child is entered iff ray_aabb_intersection(child, tmax = B) (scene.cu:109-132) holds and
 *                !(entry >= B).
 *   no exit      nothing stops early.
 * These are rt_query_occluded's predicates, which depend on (ray, B, primitive or node) alone: H is a fixed set,
 * whatever order the nodes are visited in, and rt_query_occluded returns H != {}.
 * Order: hits are sorted by the key (t', index) ascending.  t' is t's bit pattern as an unsigned integer, with
 * every NaN replaced by the one pattern 0x7FC00000.  An accepted t is NaN or >= 0.005 (the accept test lets a NaN
 * t through, as in the branchy form), so unsigned order is numeric order with the NaNs last; a NaN's sign and
 * payload are the processor's and do not influence the order.  Equal t' (two NaNs included) are ordered by index.
 * Outputs, for a caller-chosen k with 1 <= k <= RT_MULTI_HIT_MAX:
 *   count[i]                        |H| as int32, not capped by k;
 *   t[i*k + j], index[i*k + j]      the j-th smallest hit by the key, for j < min(|H|, k);
 *                                   1e30 and -1 for j >= min(|H|, k) (rt_query_closest's miss convention).
 * Every pointer of rt_multi_hit_out is optional (NULL = not written); with all three NULL the call only traverses
 * and counts (rt_query_stats).
 * Exact relations to the other calls: count >= 1 <=> rt_query_occluded with the same tmax; for B = 1e30,
 * count >= 1 <=> rt_query_closest's index >= 0.  t[0] is NOT promised to be the closest call's t: the closest
 * traversal's shrinking bound can prune a box that the fixed bound enters.
 * rt_query_multi_hit follows every rule of rt_query_occluded and rt_query_closest_hit: pointers on q's device,
 * enqueued on hip_stream, joins the event chain, allocates nothing once the scratch holds n rays (when exactly one
 * of t and index is NULL, the other's n*k list words live in a scratch of the object that grows like the rest)
 * and never waits on the host; d_out is a host struct of device pointers, read before the call returns; the
 * geometry is the object's current resident geometry (rt_query_update_triangles).  n == 0 is RT_OK and touches no
 * pointer; a null object, n < 0, k outside 1..RT_MULTI_HIT_MAX, a null d_rays or d_out with n > 0, or an n * k
 * that does not fit int32 is RT_E_INVALID before any HIP call (k is checked before n: a bad k is refused for n == 0
 * too).
 * rt_query_stats after it: live_segments = n, hits = rays with count >= 1, misses = the rest, hits_sphere = 0;
 * with collect_counters Pn/Iv/Tt and sphere_tests are the full traversal's -- no exit, so they do not depend on
 * the order and are exact on every ray.
 * The _host variant takes host pointers, stages through buffers of the object and blocks.  rt_scene_multi_hit is
 * the host twin: the same on a host scene, no GPU, bit for bit the device's output; it refuses the same bad
 * arguments. */
#define RT_MULTI_HIT_MAX 64
typedef struct {            /* every pointer optional: NULL = not written */
    float   *t;             /* n x k */
    int32_t *index;         /* n x k */
    int32_t *count;         /* n     */
} rt_multi_hit_out;
int rt_query_multi_hit(rt_query *q, const float *d_rays, const float *d_tmax /* NULL = 1e30 */, int32_t n,
                       int32_t k, const rt_multi_hit_out *d_out, void *hip_stream);
int rt_query_multi_hit_host(rt_query *q, const float *rays, const float *tmax, int32_t n, int32_t k,
                            const rt_multi_hit_out *out);
int rt_scene_multi_hit(const rt_scene *scene, const float *rays, const float *tmax, int32_t n, int32_t k,
                       const rt_multi_hit_out *out);

/* Closest-point queries: for a point, the nearest surface point, its distance and the primitive.  The
 * presence of these symbols is the feature probe; RT_ABI_VERSION and every existing struct are unchanged.  No
 * reference counterpart (the reference answers ray queries only).
 * All arithmetic is float32, each operation rounded once, no contraction; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 * points = n x {x y z} floats, contiguous; max_dist = n floats or NULL (unbounded).  S = the scene's sphere count.
 *   bound        for max_dist R: B2 = R*R if 0 <= R <= 1e18; B2 = -1 (nothing qualifies) if R < 0; otherwise (larger,
 *                +inf, NaN, or a NULL max_dist) B2 = +inf.  A point with a non-finite component is a miss and nothing
 *                is traversed (no sphere is tested either).
 *   triangle     record (p1, e1 = p2p1, e2 = p3p1), query point p: Ericson's region test on the record's own edges.
 *                  ap = p - p1;  bp = ap - e1;  cp = ap - e2
 *                  d1 = dot(e1,ap) d2 = dot(e2,ap) d3 = dot(e1,bp) d4 = dot(e2,bp) d5 = dot(e1,cp) d6 = dot(e2,cp)
 *                  vc = d1*d4 - d3*d2;  vb = d5*d2 - d1*d6;  va = d3*d6 - d5*d4
 *                (u, v) is the first of these that applies:
 *                  A     d1 <= 0 && d2 <= 0                      (0, 0)
 *                  B     d3 >= 0 && d4 <= d3                     (1, 0)
 *                  AB    vc <= 0 && d1 >= 0 && d3 <= 0           (d1 / (d1 - d3), 0)
 *                  C     d6 >= 0 && d5 <= d6                     (0, 1)
 *                  AC    vb <= 0 && d2 >= 0 && d6 <= 0           (0, d2 / (d2 - d6))
 *                  BC    va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0 w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); (1 - w, w)
 *                  face  otherwise                               den = 1 / ((va + vb) + vc); (vb * den, vc * den)
 *                point = (p1 + u*e1) + v*e2 per component; dist2 = dot(p - point, p - point).  uv means what it
 *                means in hit records: the point lies at p1 + u e1 + v e2.  A NaN dist2 (a zero-area triangle, for
 *                example) is never accepted.
 *   sphere       (c, r): w = p - c; len = sqrtf(dot(w, w)); g = len - r; dist2 = g*g; point = c + (r / len) * w per
 *                component, and c + (r, 0, 0) for len == 0; uv = (+0, +0).
 *   box          node box (lo, hi): per axis q = fmaxf(fmaxf(lo - p, p - hi), 0); box2 = (qx*qx + qy*qy) + qz*qz.
 * The walk.  The bound shrinks as primitives are accepted, so the visit order is part of the definition (as it is for
 * rt_query_closest, and unlike rt_query_occluded and rt_query_multi_hit, whose bound is fixed).  State (best2, best) =
 * (B2, INT32_MAX); the primitive with index i at dist2 is accepted, and becomes the state, iff
 * dist2 < best2 || (dist2 == best2 && i < best).
 *   1. spheres 0..S-1 in order (index k);
 *   2. if 0 > best2 stop, otherwise enter the root;
 *   3. leaf: its triangles [child2, child1) in order (index S + j), then pop;
 *   4. internal node: a = box2(child1), b = box2(child2); a child is eligible iff !(box2 > best2); child2 goes first
 *      iff it is eligible and (child1 is not, or b < a) -- a tie goes to child1; enter the first child and push the
 *      other one with its box2 if it is eligible too; with neither eligible, pop;
 *   5. pop: discard entries whose stored box2 > best2 (tested against the current state), enter the first that
 *      survives; an empty stack ends the query.
 * Outputs (rt_closest_point_out; every pointer optional, NULL = not written, all NULL = only traverse and count):
 *   distance[i] = sqrtf(best2), index[i] = best, point[i*3..], uv[i*2..] = those of the accepted primitive, evaluated
 *   once more by the same functions; a miss (nothing accepted) gives 1e30, -1, (+0, +0, +0), (+0, +0).  max_dist is
 *   inclusive: a primitive at exactly dist2 == B2 is accepted.
 * Relation to the unpruned minimum: the result is the minimum of the key (dist2, index) over the primitives the walk
 * tests, which is >= the minimum over all primitives under the same functions.  The two are equal unless a node's
 * float box2 exceeds the float dist2 of a triangle inside that box by rounding -- box2 and dist2 are rounded
 * independently, so that is possible, and the walk then prunes the box; the answer is then farther than the true
 * nearest point by rounding error only (DESIGN §15 has the measured bound).
 * rt_query_closest_point follows every rule of rt_query_multi_hit: pointers on q's device, enqueued on hip_stream,
 * joins the event chain, allocates nothing once the scratch holds n points (rt_query_reserve counts points like rays)
 * and never waits on the host; d_out is a host struct of device pointers, read before the call returns; the geometry
 * is the object's current resident geometry (rt_query_update_triangles).  n == 0 is RT_OK and touches no pointer; a
 * null object, n < 0, or a null d_points or d_out with n > 0 is RT_E_INVALID before any HIP call.
 * rt_query_stats after it: live_segments = n, hits = queries with index >= 0, misses = the rest, hits_sphere = those
 * whose nearest primitive is a sphere; with collect_counters Pn = nodes entered (the root, each child entered, each
 * popped entry that survives), Iv = internal nodes visited, Tt = triangle tests, and sphere_tests -- all exact,
 * because the order is pinned.
 * The _host variant takes host pointers, stages through buffers of the object and blocks.  rt_scene_closest_point is
 * the host twin: the same walk over rt_scene.bvh on a host scene, no GPU, bit for bit the device's output (or NaN on
 * both sides); it refuses the same bad arguments. */
typedef struct {            /* every pointer optional: NULL = not written */
    float   *distance;      /* n     */
    int32_t *index;         /* n     */
    float   *point;         /* n x 3 */
    float   *uv;            /* n x 2 */
} rt_closest_point_out;
int rt_query_closest_point(rt_query *q, const float *d_points, const float *d_max_dist /* NULL = unbounded */,
                           int32_t n, const rt_closest_point_out *d_out, void *hip_stream);
int rt_query_closest_point_host(rt_query *q, const float *points, const float *max_dist, int32_t n,
                                const rt_closest_point_out *out);
int rt_scene_closest_point(const rt_scene *scene, const float *points, const float *max_dist, int32_t n,
                           const rt_closest_point_out *out);

/* Range queries: for a point, every primitive within max_dist -- the K nearest in order, and their count.
 * The presence of these symbols is the feature probe; RT_ABI_VERSION and every existing struct are unchanged.  No
 * reference counterpart.  This is to rt_query_closest_point what rt_query_multi_hit is to rt_query_closest.
 * All arithmetic is the closest-point block's above (bound, triangle, sphere, box: host/closest_point_math.h is the only
 * statement of it).  points, max_dist and S as there.
 *   bound        B2 of max_dist[i] by the closest-point rule: R*R for 0 <= R <= 1e18, -1 for R < 0, +inf otherwise
 *                (larger, +inf, NaN, or a NULL max_dist).  A point with a non-finite component has count = 0 and
 *                nothing is tested.
 * H is the set of primitives found with the bound HELD at B2:
 *   spheres      every sphere j is tested (sphere dist2); it is a member, with index j, iff dist2 <= B2.
 *   root         entered iff !(0 > B2).
 *   leaf         in an entered leaf every triangle j of [child2, child1) is tested (triangle dist2); it is a member,
 *                with index S + j, iff dist2 <= B2.  A NaN dist2 never qualifies.
 *   internal     a child is entered iff !(box2(child) > B2).
 *   no exit      nothing stops early and the bound never shrinks.
 * Every predicate depends on (point, B2, primitive or node) alone, so H is a fixed set whatever order the nodes are
 * visited in -- the argument made for rt_query_occluded and rt_query_multi_hit.  It does not hold for
 * rt_query_closest_point: there the bound is the best distance so far, which nodes are entered depends on what was
 * accepted before, and the visit order is part of that call's definition.
 * Order: members are sorted by the key (dist2's bit pattern as uint32, index) ascending.  A member's dist2 is a sum of
 * squares, >= +0 and not NaN, so unsigned order is numeric order; equal dist2 goes to the smaller index.
 * Outputs, for a caller-chosen k with 1 <= k <= RT_NEAREST_K_MAX (every pointer optional, NULL = not written; with all
 * NULL the call only traverses and counts):
 *   count[i]                 |H| as int32, not capped by k;
 *   entry j < min(|H|, k)    of row i (distance[i*k + j], index[i*k + j], point[(i*k + j)*3..]): the j-th member by the
 *                            key: sqrtf(dist2), its index, and its nearest point, evaluated once more by the triangle
 *                            or sphere rule as rt_query_closest_point does;
 *   entry j >= min(|H|, k)   1e30, -1, (+0, +0, +0).
 * Exact relations to rt_query_closest_point with the same max_dist:
 *   1. count >= 1 <=> its index >= 0: before its first accept that walk enters exactly the nodes this one enters.
 *   2. the key of entry 0 is <= the key of its answer: it tests a subset of what the held bound tests; the two are
 *      equal wherever its pruning did not slip by rounding.
 *   3. H is a subset of the brute-force set {dist2 <= B2} over all primitives under the same functions; a primitive of
 *      that set missing from H has an ancestor node whose float box2 > B2 (box2 and dist2 are rounded independently),
 *      and that is the only way the two differ.
 * rt_query_nearest_k follows every rule of rt_query_multi_hit: pointers on q's device, enqueued on hip_stream, joins
 * the event chain, allocates nothing once the scratch holds n points (rt_query_reserve counts points; when distance or
 * index is NULL but a list is needed -- any of distance, index, point given -- the missing half's n*k words live in
 * the object's multi-hit list scratch, which grows the same way) and never waits on the host; d_out is a host struct
 * of device pointers, read before the call returns; the geometry is the object's current resident geometry
 * (rt_query_update_triangles).  n == 0 is RT_OK and touches no pointer; a null object (or scene), n < 0, k outside
 * 1..RT_NEAREST_K_MAX (checked before n == 0, as rt_query_multi_hit does), a null points or out pointer with n > 0, or
 * an n * k that does not fit int32 is RT_E_INVALID before any HIP call.
 * rt_query_stats after it: live_segments = n, hits = queries with count >= 1, misses = the rest, hits_sphere = 0; with
 * collect_counters Pn (nodes entered), Iv, Tt and sphere_tests are the full walk's -- order-independent, exact on every
 * query.
 * The _host variant takes host pointers, stages through buffers of the object and blocks.  rt_scene_nearest_k is the
 * host twin: the same on a host scene (rt_scene.bvh), no GPU, bit for bit the device's output; it refuses the same bad
 * arguments. */
#define RT_NEAREST_K_MAX 64
typedef struct {            /* every pointer optional: NULL = not written */
    float   *distance;      /* n x k     */
    int32_t *index;         /* n x k     */
    float   *point;         /* n x k x 3 */
    int32_t *count;         /* n         */
} rt_nearest_k_out;
int rt_query_nearest_k(rt_query *q, const float *d_points, const float *d_max_dist /* NULL = unbounded */,
                       int32_t n, int32_t k, const rt_nearest_k_out *d_out, void *hip_stream);
int rt_query_nearest_k_host(rt_query *q, const float *points, const float *max_dist, int32_t n, int32_t k,
                            const rt_nearest_k_out *out);
int rt_scene_nearest_k(const rt_scene *scene, const float *points, const float *max_dist, int32_t n, int32_t k,
                       const rt_nearest_k_out *out);

/* Filtered ray queries: the closest hit and the any-hit answer over the surfaces the caller lets count -- a per-ray
 * interval, one primitive to skip and visibility masks.  The presence of these symbols is the feature
 * probe; RT_ABI_VERSION and every existing struct are unchanged.  No reference counterpart as an interface; every
 * geometric predicate restates the reference's traversal.
 * All arithmetic is float32, each operation rounded once, no contraction.  S = the scene's sphere count, T its
 * triangle count; primitives are numbered as everywhere (spheres first, then S + triangle).
 * rt_ray_filter: one optional array of n entries per member (NULL = not given); a NULL struct behaves as a struct of
 * NULLs.  For ray i:
 *   lower bound  lo = tmin[i] > kEps ? tmin[i] : kEps, kEps = 0.005 as a float (0x1.47ae16p-8): NULL, NaN, negative and
 *                small values give kEps, the unfiltered calls' behaviour; with +inf nothing is accepted.
 *   upper bound  B by rt_query_occluded's rule: tmax[i] where tmax[i] <= 1e30, otherwise (larger, +inf, NaN, NULL) 1e30.
 *   masks        the object holds an optional array M of S + T uint32 words in the primitive numbering
 *                (rt_query_set_masks); with none set every primitive's word is 0xFFFFFFFF.  The ray's word is
 *                rm = mask ? mask[i] : 0xFFFFFFFF.
 *   eligible(p)  (p != skip[i]) && ((M[p] & rm) != 0).  A skip value that names no primitive, and a NULL skip, exclude
 *                nothing; rm = 0 excludes everything.
 *   triangle j   accepted under a bound c iff the reference's test (scene.cu:160-195) accepts with closest = c, giving
 *                t, and !(t < lo), and eligible(S + j).  Because lo >= kEps this equals the reference's test with kEps
 *                replaced by lo.
 *   sphere k     the reference's test (scene.cu:340-371) with kEps replaced by lo: the near root t = mhb - hs if
 *                t < c && !(t < lo), otherwise the far root t = mhb + hs under the same test; accepted iff one of them
 *                passes and eligible(k).  A lo between the two roots therefore returns the far root.  With lo = kEps
 *                this is the reference's test bit for bit.  host/ray_filter_math.h is the only statement of it.
 * rt_query_occluded_filtered is rt_query_occluded's definition with these acceptance tests: `closest` is held at B, the
 * root is entered iff !(0 >= B), a child iff its box is hit with tmax = B and !(entry >= B), and the answer is 1 iff
 * some primitive is accepted.  Eligibility depends on the ray and the primitive alone and the bound is held, so which
 * nodes are entered does not depend on the visit order and neither does the answer -- rt_query_occluded's argument,
 * unchanged.  With a NULL filter and no masks it is rt_query_occluded bit for bit, counters included.
 * rt_query_closest_filtered has a pinned walk of its own, part of the call's definition (the bound shrinks, so the order
 * matters, as for rt_query_closest; unlike that call the near child goes first).  State closest = B, index = -1.
 *   1. spheres 0..S-1 in order, each tested under the current closest; an accepted one sets closest = t, index = k;
 *   2. if 0 >= closest the ray ends (no node is entered), otherwise the root is entered;
 *   3. leaf: its triangles [child2, child1) in order under the current closest; an accepted one sets closest = t,
 *      index = S + j; the exhausted leaf pops;
 *   4. internal node: ray_aabb_intersection (scene.cu:109-132) of child1, then of child2, with tmax = closest; a child is
 *      entered iff it is hit and !(entry >= closest); child2 goes first iff it is entered and (child1 is not, or
 *      t2 < t1) -- a tie goes to child1; the selected child is entered and, if both are entered, the other one is
 *      pushed with its entry distance; with neither entered, pop;
 *   5. pop: an empty stack ends the ray; an entry whose stored distance >= the current closest is discarded and the walk
 *      pops again; otherwise it is entered.
 * Result: (closest, index), and (1e30, -1) when nothing was accepted.  A NaN follows the predicates literally, as in
 * the reference: an accepted NaN t becomes closest.  The walk pushes at most one entry per level.
 * Relations, under one filter and one set of masks:
 *   R1  index >= 0 <=> rt_query_occluded_filtered == 1: until its first accept the walk's bound is B and it enters
 *       exactly the nodes the any-hit walk enters.
 *   R2  a hit (t, index) is a member of the brute-force set {p eligible, accepted under the bound B}.
 *   R3  it is NOT promised to be that set's minimum, nor, with an empty filter, rt_query_closest's answer: a box's float
 *       entry distance can exceed the float t of a triangle inside it, either shrinking-bound walk then prunes the box,
 *       and the two walks break exact-t ties by their own visit order (DESIGN §17 has the measured counts).
 * rt_query_set_masks copies count = S + T words from a device pointer into a buffer of the object on hip_stream and
 * joins the event chain: calls enqueued earlier see the old masks, later ones the new; NULL drops the masks (count is
 * still checked).  The masks survive rt_query_update_triangles.  After it, with no query since, rt_query_stats returns
 * zeros.  The _host variant takes a host pointer and blocks.
 * The two query calls follow every rule of rt_query_multi_hit: device pointers on q's device, enqueued on hip_stream,
 * they join the event chain, allocate nothing once the scratch holds n rays and never wait on the host; d_filter and
 * d_out are host structs of device pointers, read before the call returns; the geometry is the object's current
 * resident geometry.  rt_query_closest_filtered writes any field of rt_hit_out, all optional, the record being
 * rt_query_closest_hit's of the filtered (t, index).  n == 0 is RT_OK and touches no pointer; a null object or scene,
 * n < 0, null rays or a null output with n > 0, or a count other than S + T is RT_E_INVALID before any HIP call.
 * rt_query_stats after them reports as after rt_query_closest and rt_query_occluded; with collect_counters Pn (nodes
 * entered), Iv, Tt and sphere_tests are those of the pinned walks, exact on every ray (the any-hit walk stops at its
 * first accept, the closest one tests every sphere).
 * The _host variants take host pointers throughout (the filter's members too), stage through buffers of the object and
 * block.  rt_scene_closest_filtered and rt_scene_occluded_filtered are the host twins: the same walks over rt_scene.bvh
 * on a host scene, no GPU, bit for bit the device's output; masks = S + T host words or NULL; stats (optional) receives
 * live_segments, hits, misses, hits_sphere (closest) and the four counters.  The hit-record fields of a filtered hit
 * on the host are rt_scene_hit_records applied to the twin's (t, index). */
typedef struct {            /* every pointer optional: NULL = not given */
    const float    *tmin;   /* n */
    const float    *tmax;   /* n */
    const int32_t  *skip;   /* n */
    const uint32_t *mask;   /* n */
} rt_ray_filter;
int rt_query_set_masks(rt_query *q, const uint32_t *d_masks /* NULL: none */, int32_t count, void *hip_stream);
int rt_query_set_masks_host(rt_query *q, const uint32_t *masks, int32_t count);
int rt_query_closest_filtered(rt_query *q, const float *d_rays, const rt_ray_filter *d_filter, int32_t n,
                              const rt_hit_out *d_out, void *hip_stream);
int rt_query_occluded_filtered(rt_query *q, const float *d_rays, const rt_ray_filter *d_filter, int32_t n,
                               uint8_t *d_occluded, void *hip_stream);
int rt_query_closest_filtered_host(rt_query *q, const float *rays, const rt_ray_filter *filter, int32_t n,
                                   const rt_hit_out *out);
int rt_query_occluded_filtered_host(rt_query *q, const float *rays, const rt_ray_filter *filter, int32_t n,
                                    uint8_t *occluded);
int rt_scene_closest_filtered(const rt_scene *scene, const uint32_t *masks, const float *rays,
                              const rt_ray_filter *filter, int32_t n, float *t, int32_t *index, rt_stats *stats);
int rt_scene_occluded_filtered(const rt_scene *scene, const uint32_t *masks, const float *rays,
                               const rt_ray_filter *filter, int32_t n, uint8_t *occluded, rt_stats *stats);

/* Hemisphere visibility queries: how many of S sample rays over the hemisphere above a surface point escape -- ambient
 * occlusion, sky visibility, lightmap and probe baking.  The presence of these symbols is the feature probe;
 * RT_ABI_VERSION and every existing struct are unchanged.  No reference counterpart as an interface; the sample
 * generator is built from the reference's pcg, random_on_sphere and normalise, the walk is rt_query_occluded_filtered's.
 * Inputs: frames, n rows of 6 floats {p.xyz, nrm.xyz} (a ray's layout); an optional rt_ray_filter of n entries, row i
 * applying to every sample of point i (skip keeps a point on a surface off its own triangle, tmax is the AO radius; NULL
 * = the defaults); params: samples = S in 1..RT_HEMISPHERE_MAX_SAMPLES with n * S <= 2^31 - 1, mode, seed, point_offset.
 * The sample ray of work item (i, s), 0 <= s < S; all arithmetic float32, each operation rounded once, no contraction;
 * host/hemisphere_math.h is the only statement of it:
 *   nh  = normalise(nrm) = (1.0f / sqrtf(magsq(nrm))) * nrm; a zero or non-finite normal gives what the arithmetic gives;
 *   w   = (point_offset + i) * S + s in uint32 arithmetic (it wraps);
 *   rng = pcg_seed(w * 0x9E3779B1u + seed * 0x85EBCA6Bu);  u = random_on_sphere(rng);
 *   RT_HEMISPHERE_COSINE   v = nh + u, m = magsq(v), dir = !(m >= 0x1p-40f) ? nh : (1.0f / sqrtf(m)) * v;
 *   RT_HEMISPHERE_UNIFORM  dir = dot(u, nh) < 0 ? -u : u;
 *   the ray is (p, dir).
 * point_offset lets a caller split a batch: rows [a, b) called with point_offset = a give the whole batch's rows.
 * Answer: open_count[i] = the number of point i's S rays for which rt_query_occluded_filtered's definition, under filter
 * row i and the object's masks, answers 0 (int32); openness[i] = (float)open_count[i] / (float)S by IEEE division.  Both
 * are optional members of rt_hemisphere_out.  The count is an integer and the any-hit answer does not depend on the
 * visit order, so the result is exactly reproducible.
 * rt_query_hemisphere follows every rule of rt_query_occluded_filtered: device pointers on q's device, enqueued on
 * hip_stream, it joins the event chain, allocates nothing once the scratch holds n points (rt_query_reserve counts
 * points: the scratch grows with n, 44 bytes per point, not with n * S) and never waits on the host; d_filter, params and
 * d_out are host structs, read before the call returns; the geometry and the masks are the object's current ones.
 * n == 0 is RT_OK and touches no pointer, params included; a null object or scene, n < 0, and with n > 0 null frames,
 * null params, S outside 1..RT_HEMISPHERE_MAX_SAMPLES, an unknown mode, n * S > 2^31 - 1, or a null out or both outputs
 * null is RT_E_INVALID with a message before any HIP call.
 * rt_query_stats after it: live_segments = n * S, hits = occluded samples, misses = escaped samples; with
 * collect_counters Pn, Iv, Tt and sphere_tests are the pinned any-hit walk's, summed over all n * S rays, exact.
 * The _host variant takes host pointers throughout, stages through buffers of the object and blocks.
 * rt_scene_hemisphere is the host twin: the same on a host scene (rt_scene.bvh), no GPU, bit for bit the device's output;
 * masks = S + T host words or NULL; stats is optional.  rt_hemisphere_rays writes the n * S x 6 sample rays a call stands
 * for (host only, no scene): row i * S + s = (p_i, dir(i, s)). */
#define RT_HEMISPHERE_MAX_SAMPLES 4096
#define RT_HEMISPHERE_COSINE  0
#define RT_HEMISPHERE_UNIFORM 1
typedef struct {
    int32_t  samples;       /* S */
    int32_t  mode;          /* RT_HEMISPHERE_COSINE or RT_HEMISPHERE_UNIFORM */
    uint32_t seed;
    uint32_t point_offset;
} rt_hemisphere_params;
typedef struct {            /* every pointer optional: NULL = not written; at least one with n > 0 */
    int32_t *open_count;    /* n */
    float   *openness;      /* n */
} rt_hemisphere_out;
int rt_query_hemisphere(rt_query *q, const float *d_frames, const rt_ray_filter *d_filter, int32_t n,
                        const rt_hemisphere_params *params, const rt_hemisphere_out *d_out, void *hip_stream);
int rt_query_hemisphere_host(rt_query *q, const float *frames, const rt_ray_filter *filter, int32_t n,
                             const rt_hemisphere_params *params, const rt_hemisphere_out *out);
int rt_scene_hemisphere(const rt_scene *scene, const uint32_t *masks, const float *frames, const rt_ray_filter *filter,
                        int32_t n, const rt_hemisphere_params *params, const rt_hemisphere_out *out, rt_stats *stats);
int rt_hemisphere_rays(const float *frames, int32_t n, const rt_hemisphere_params *params, float *rays_out);

/* Box overlap queries: for an axis-aligned box, every primitive whose surface meets it -- the K smallest indices in
 * order, their count and an any flag: collision broad phase, voxelisation, trigger volumes, region picking.
 * The presence of these symbols is the feature probe; RT_ABI_VERSION and every existing struct are unchanged.  No
 * reference counterpart.
 * All arithmetic is float32, each operation rounded once, no contraction; host/box_overlap_math.h is the only statement
 * of it.  S = the scene's sphere count; primitives are numbered as everywhere (spheres first, then S + triangle).
 * boxes: n rows of 6 floats {lo.xyz, hi.xyz}.
 *   valid box    all six numbers finite and lo.c <= hi.c on every axis.  A box that is not valid has count = 0, any = 0 and
 *                a row of padding; nothing is tested for it and it adds nothing to the counters.
 *   surfaces     only surfaces count, as for rt_query_closest_point: a box strictly inside a closed mesh or inside a
 *                sphere meets nothing.
 *   node         boxes_meet(nlo, nhi, lo, hi): on every axis nlo.c <= hi.c && lo.c <= nhi.c.  Comparisons only, closed
 *                (touching counts); the empty-box sentinel meets nothing.
 *   triangle     (p1, e1 = p2p1, e2 = p3p1), vertices v0 = p1, v1 = p1 + e1, v2 = p1 + e2 (one rounding per component): a
 *                member iff none of 13 axes separates.  1-3, the box axes: the min / max of the three vertices'
 *                coordinate c separates iff tmin > hi.c || tmax < lo.c.  4, the plane: m = cross(e1, e2) (each component
 *                a*b - c*d; not the stored unit normal), s = dot(m, v0) = (m.x*v0.x + m.y*v0.y) + m.z*v0.z,
 *                bmin = (fminf(m.x*lo.x, m.x*hi.x) + fminf(m.y*lo.y, m.y*hi.y)) + fminf(m.z*lo.z, m.z*hi.z), bmax the same
 *                with fmaxf; separates iff s < bmin || s > bmax.  5-13, a = edge x unit_i for the edges e1, e2, e2 - e1
 *                and i = x, y, z in that order for each: with a's two non-zero components (a1, a2) on coordinates
 *                (c1, c2) -- x: (f.z, -f.y) on (y, z); y: (-f.z, f.x) on (x, z); z: (f.y, -f.x) on (x, y) -- a vertex
 *                projects to a1*v.c1 + a2*v.c2, the box to [fminf(a1*lo.c1, a1*hi.c1) + fminf(a2*lo.c2, a2*hi.c2), the
 *                same with fmaxf]; separates iff tmin > bmax || tmax < bmin.  Every separating comparison is strict: a
 *                NaN never separates, and a zero axis projects everything to 0 and never separates.
 *   sphere       (c, r): near2 = the closest-point block's box2(c, lo, hi); far2 = (fx*fx + fy*fy) + fz*fz with
 *                f.c = fmaxf(fabsf(c.c - lo.c), fabsf(hi.c - c.c)); a member iff near2 <= r*r && far2 >= r*r.
 * H, the set of a valid box: every sphere j is tested, a member with index j; the root is entered; in an entered leaf
 * every triangle j of [child2, child1) is tested, a member with index S + j; a child is entered iff boxes_meet(child box,
 * box); nothing stops early.  Every predicate depends on (box, primitive or node) alone, so H is a fixed set whatever
 * order the nodes are visited in -- rt_query_nearest_k's argument.
 * Outputs, for a caller-chosen k with 1 <= k <= RT_OVERLAP_K_MAX (every pointer optional, NULL = not written):
 *   count[i]   |H| as int32, not capped by k;
 *   any[i]     1 iff |H| >= 1, else 0;
 *   index      row i holds the min(|H|, k) smallest member indices ascending, then -1.
 * The any-only walk: with only `any` given (index and count NULL) the walk of a box stops at its first member.  The
 * answer does not depend on the order; the counters do, so the order is pinned and part of the definition, as
 * rt_query_occluded's is: spheres in order; the root; in a leaf, triangles in order; at an internal node child1 is
 * entered if it meets, else child2, and child2 is pushed when both meet; a pop enters the popped node.  The full walk
 * uses the same order, but its counters do not depend on it.
 * Relation to brute force (every primitive under triangle / sphere above): H is a subset of that set; a member of it
 * missing from H has an ancestor node whose box fails boxes_meet.  That can happen by an ulp -- node boxes are grown
 * from the loaded vertices (and by rt_scene_refit / rt_query_update_triangles from the given ones), while the test sees
 * p1 + e1 -- and it is the only way the two sets differ.
 * rt_query_overlap_box follows every rule of rt_query_nearest_k: pointers on q's device, enqueued on hip_stream, joins the
 * event chain, allocates nothing once the scratch holds n boxes (rt_query_reserve counts boxes) and never waits on the
 * host; d_out is a host struct of device pointers, read before the call returns; the geometry is the object's current
 * resident geometry (rt_query_update_triangles).  n == 0 is RT_OK and touches no pointer; a null object (or scene),
 * n < 0, k outside 1..RT_OVERLAP_K_MAX (checked before n == 0), a null boxes or out pointer with n > 0, or an n * k that
 * does not fit int32 is RT_E_INVALID before any HIP call.
 * rt_query_stats after it: live_segments = n, hits = boxes with a member, misses = the rest, hits_sphere = 0; with
 * collect_counters Pn (nodes entered), Iv, Tt and sphere_tests are those of the walk that ran (the any-only one stops
 * early), exact in both modes.
 * The _host variant takes host pointers, stages through buffers of the object and blocks.  rt_scene_overlap_box is the
 * host twin: the same on a host scene (rt_scene.bvh), no GPU, bit for bit the device's output; it refuses the same bad
 * arguments. */
#define RT_OVERLAP_K_MAX 64
typedef struct {            /* every pointer optional: NULL = not written */
    int32_t *index;         /* n x k */
    int32_t *count;         /* n     */
    uint8_t *any;           /* n     */
} rt_overlap_out;
int rt_query_overlap_box(rt_query *q, const float *d_boxes, int32_t n, int32_t k, const rt_overlap_out *d_out,
                         void *hip_stream);
int rt_query_overlap_box_host(rt_query *q, const float *boxes, int32_t n, int32_t k, const rt_overlap_out *out);
int rt_scene_overlap_box(const rt_scene *scene, const float *boxes, int32_t n, int32_t k, const rt_overlap_out *out);

/* ------------------------------------------------------------------ scenes from vertex and index arrays
 * rt_scene_from_mesh makes an rt_scene_host from arrays instead of a scene file, and rt_scene_face_index tells which
 * input triangle each scene triangle is.  The presence of these symbols is the feature probe;
 * RT_ABI_VERSION and every existing struct are unchanged.  No reference counterpart.
 * Definition by equivalence -- the whole contract: the scene is byte for byte (every array and every scalar field of
 * the rt_scene view: min_coord, inv_dimensions, the camera precompute, exposure, ...) the one rt_scene_load produces for
 * the description's canonical scene file, whose lines are, in this order:
 *   material m<k> diffuse r g b specular r g b emit r g b metallicity f roughness f ior f     per material, in order;
 *   sky r g b                                                                                 if a sky is given;
 *   sphere m<k> cx cy cz r                                                                    per sphere;
 *   triangle m<k> <nine floats>                                                               per triangle, input order;
 *   camera position x y z forward x y z up x y z fov deg                                      if a camera is given;
 * every float printed so that it parses back to itself.  Width, height, spp, bounces and exposure come from opts
 * (image_override, exposure_override), else the loader's defaults (1920 1080 1 3, exposure 0).  So: the triangle order
 * and the node array are the reference build's; forward and up are normalised as the loader normalises them; the fov
 * is (float)(deg * (pi / 180)) with the product in double; use_bvh = 0 gives the single leaf; bvh_device chooses the
 * builder and does not change a bit.  Environment maps from memory are not offered (no query reads the sky).
 * Refusals, all RT_E_INVALID, rt_last_error names the primitive, before either builder runs and, in the host entry,
 * before any HIP call; in this order: a null mesh or out; a negative count; vertices NULL with triangle_count > 0
 * (spheres NULL with sphere_count > 0); a soup whose vertex_count != 3 * triangle_count; a material-index array without
 * a material table; material_count > 65535; sphere_count + triangle_count past int32; the loader's image-size rule; a
 * sphere's, then a triangle's material index >= material_count (the first such); a vertex index < 0 or >= vertex_count
 * (the smallest such triangle; before any finiteness check); then the loader's own rules with its own messages: a
 * non-finite sphere; the first triangle in input order with a non-finite vertex coordinate or, its coordinates being
 * finite, a non-finite centroid.  A non-finite vertex that no triangle references is not an error.
 * rt_scene_from_mesh_device: vertices, indices and triangle_materials are device pointers on device
 * opts->bvh_device, which must be >= 0 (else RT_E_INVALID); spheres, materials, camera and sky stay host memory.  The
 * call is synchronous: it synchronises hip_stream (NULL = the null stream) before its first kernel reads the arrays,
 * assembles, validates, builds and finalises on the device (csrc/mesh_ingest.hip, csrc/bvh_build.hip) and downloads
 * the result.  What it returns is an ordinary host-owned rt_scene_host -- the scene does not stay on the device: the
 * host twins (rt_scene_*) and rt_query_create's record packing read the arrays on the host.  Same result, same
 * refusals and same messages as the host entry on the same numbers.
 * rt_scene_face_index: a borrowed array of triangle_count int32, valid until rt_scene_free; entry j is the input index
 * of scene triangle j, which is answer index sphere_count + j of every query.  Every rt_scene_host has it; for a
 * file-loaded scene the input index is the triangle's position in the file (quads and ply faces counted as the
 * triangles they become).  rt_scene_refit leaves it alone. */
typedef struct { rt_vec3 position, forward, up; float vertical_fov_degrees; } rt_camera_desc;
typedef struct {
    const float   *vertices;  int32_t vertex_count;     /* 3 floats each */
    const int32_t *indices;   int32_t triangle_count;   /* 3 per triangle; NULL = soup: triangle i is
                                                           vertices 3i, 3i+1, 3i+2 and vertex_count == 3*triangle_count */
    const uint16_t *triangle_materials;                 /* per triangle; NULL = all 0 */
    const rt_sphere *spheres; int32_t sphere_count; const uint16_t *sphere_materials; /* NULL = all 0 */
    const rt_material *materials; int32_t material_count; /* NULL/0 = one material: the loader's default
                                                           (diffuse and specular 1,1,1, everything else 0) */
    const rt_camera_desc *camera;                       /* NULL = what a file without a `camera` line gives */
    const rt_vec3 *sky;                                 /* NULL = what a file without `sky` gives (one 0 texel) */
} rt_mesh_desc;
int rt_scene_from_mesh(const rt_mesh_desc *mesh, const rt_load_opts *opts, rt_scene_host **out);
int rt_scene_from_mesh_device(const rt_mesh_desc *mesh, const rt_load_opts *opts, void *hip_stream, rt_scene_host **out);
int rt_scene_face_index(const rt_scene_host *scene, const int32_t **index_out, int32_t *count_out);

/* Replaces the bloom block of main (raytracing.cu:356-393, kernels :21-74): high-pass
 * (luminance > threshold), clamped box blur of `radius` horizontally then vertically,
 * add back.  fb is a host W*H*3 buffer, updated in place. */
int rt_bloom(float *fb, int32_t width, int32_t height, float threshold, int32_t radius, int32_t device);
/* Same on a device-resident framebuffer (device pointer). */
int rt_bloom_device(float *d_fb, int32_t width, int32_t height, float threshold, int32_t radius,
                    int32_t device);

/* Replaces write_framebuffer_to_output_image (raytracing.cu:286-303). rgb_out: W*H*3. */
void rt_tonemap(const float *fb, int32_t width, int32_t height, float exposure, int32_t ray_count,
                uint8_t *rgb_out);
/* Replaces stbi_write_png (raytracing.cu:395): 8-bit RGB PNG, own encoder (lossless). */
int rt_write_png(const char *path, const uint8_t *rgb, int32_t width, int32_t height);

/* Replaces `Vec3 *cpu_raytrace(Scene *scene)` (raytracing.cu:122-163): the reference's
 * OpenMP CPU path with its bounce-invariant seed; fb_out W*H*3 (overwritten).  Returns the
 * number of passes rendered; seconds = the "CPU Took" span. */
int rt_cpu_render(const rt_scene *scene, float *fb_out, int32_t threads, double *seconds);

const char *rt_last_error(void);
int rt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_ABI_H */
