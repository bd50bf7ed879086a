/*
 * kt_abi.h -- C-ABI of libkt_hip.so: the MI355X (gfx950) replacement for Kintinuous's device operator
 * API.  The reference has no FFI; its seam is the header src/frontend/cuda/internal.h:295-536 (free
 * functions over DeviceArray2D / PtrStep views, implemented in src/frontend/cuda/ *.cu) plus the
 * container classes in src/frontend/cuda/containers/.  Each entry point below names the reference
 * function it replaces.  kintinuous_amd/host/internal.h re-creates the reference's C++ names as inline
 * wrappers over these calls.
 *
 * Conventions
 *   - every function returns an int status: KT_OK (0) or a KT_ERR_* code; kt_last_error() gives the text.
 *     (The reference prints and exit(0)s on any CUDA error, internal.h:76-86; the C++ wrappers keep that.)
 *   - all image / map / volume pointers are DEVICE pointers (hipMalloc'ed: kt_malloc, or any other HIP
 *     allocation, e.g. a torch tensor's data_ptr) unless the parameter name ends in _host.
 *   - all buffers are dense: row pitch == cols * sizeof(T)  (the reference's volume kernels assume it,
 *     tsdf_volume.cu:612; reduce.cu:444,767).
 *   - vmap / nmap: float[3*rows][cols] (x, y, z planes stacked by rows; invalid = NaN in the x plane).
 *   - tsdf volume: int16[N^3], index x + y*N + z*N*N, storage wrapped by voxel_wrap (tsdf_volume.cu:612);
 *     colour volume: uint8[N^3][4] = r, g, b, weight (the voxel weight lives in .w).
 *   - VOL (internal.h:243) and the image resolution are runtime parameters (N, cols, rows).
 *   - work is enqueued on the context's HIP stream; functions with *_host outputs synchronise that stream
 *     before returning, the others return right after the launch (call kt_sync to wait).
 *   - not thread-safe per context; use one context per host thread / per GPU (the reference is single
 *     GPU-thread too).
 */
#ifndef KT_ABI_H_
#define KT_ABI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KT_OK 0
#define KT_ERR_HIP 1      /* a HIP runtime call or launch failed */
#define KT_ERR_ARG 2      /* bad argument */
#define KT_ERR_NOMEM 3
#define KT_ERR_STATE 4
#define KT_ERR_CAPACITY 5 /* an output did not fit its buffer: nothing was written past it, the true sizes were returned */

typedef struct kt_ctx kt_ctx;

typedef struct { float fx, fy, cx, cy; } kt_intr;   /* Intr, internal.h:249-260 */
typedef struct { float m[9]; } kt_mat33;            /* Mat33, internal.h:279-282, row-major */
typedef struct { float v[29]; } kt_jtj;             /* JtJJtrSE3, internal.h:98-149 */
typedef struct {                                    /* DataTerm, internal.h:90-96 (16 bytes) */
    int16_t zero_x, zero_y, one_x, one_y;
    float diff;
    uint8_t valid, pad[3];
} kt_dataterm;
typedef struct {                                    /* PointXYZRGB, internal.h:156-184 (32 bytes) */
    float x, y, z, pad0;
    uint8_t b, g, r, a;
    uint32_t pad1[3];
} kt_point_xyzrgb;
/* internal.h:186-229 == pcl::PointXYZRGBNormal (48 bytes): what CloudSliceProcessor fills CloudSlice::processedCloud with */
typedef struct {
    float x, y, z, pad0;                    /* data[3] = 1 */
    float normal_x, normal_y, normal_z, pad1;
    uint8_t b, g, r, a;
    float curvature;
    float pad2[2];
} kt_point_xyzrgbnormal;
/* a vertex of the mesh stage (kt_extract_mesh, 16 bytes): rgb packed like kt_point_xyzrgb's b, g, r, a bytes (a = weight) */
typedef struct {
    float x, y, z;
    uint32_t rgb;
} kt_mesh_vertex;

/* ---- context / memory: replaces containers/device_memory.cpp, initialization.cpp, cudaSetDevice ---- */
const char* kt_last_error(void);
const char* kt_version(void);
int kt_device_count(int* count);
int kt_ctx_create(int device, kt_ctx** out);           /* cudaSetDevice(gpu) TrackerInterface.cpp:48 + a private stream */
int kt_ctx_destroy(kt_ctx* ctx);
int kt_ctx_set_stream(kt_ctx* ctx, void* hip_stream);  /* run on a caller-owned hipStream_t (e.g. torch's) */
void* kt_ctx_stream(kt_ctx* ctx);
int kt_sync(kt_ctx* ctx);                              /* cudaDeviceSynchronize at the end of the reference wrappers */
int kt_malloc(kt_ctx* ctx, size_t bytes, void** dptr); /* DeviceMemory::create  device_memory.cpp:98-117 */
int kt_free(kt_ctx* ctx, void* dptr);                  /* DeviceMemory::release */
int kt_memset(kt_ctx* ctx, void* dptr, int value, size_t bytes);
int kt_upload(kt_ctx* ctx, void* dst, const void* src_host, size_t bytes);      /* DeviceMemory::upload */
int kt_download(kt_ctx* ctx, void* dst_host, const void* src, size_t bytes);    /* DeviceMemory::download */
/* DeviceMemory2D::upload/download with a host pitch (device side dense)  device_memory.cpp:206-227 */
int kt_upload2d(kt_ctx* ctx, void* dst, const void* src_host, size_t host_pitch, size_t row_bytes, int rows);
int kt_download2d(kt_ctx* ctx, void* dst_host, size_t host_pitch, const void* src, size_t row_bytes, int rows);

/* ---- image-side kernels ---- */
/* bilateralFilter  internal.h:299 / bilateral_pyrdown.cu:332-342 */
int kt_bilateral_filter(kt_ctx* ctx, const uint16_t* src, uint16_t* dst, int cols, int rows);
/* pyrDown  internal.h:307 / bilateral_pyrdown.cu:344-354; dst is (scols/2) x (srows/2) */
int kt_pyr_down(kt_ctx* ctx, const uint16_t* src, int scols, int srows, uint16_t* dst);
/* createVMap  internal.h:328 / maps.cu:122-137 */
int kt_create_vmap(kt_ctx* ctx, const kt_intr* intr, const uint16_t* depth, int cols, int rows, float* vmap);
/* createNMap  internal.h:335 / maps.cu:139-154 */
int kt_create_nmap(kt_ctx* ctx, const float* vmap, int cols, int rows, float* nmap);
/* tranformMaps  internal.h:346 / maps.cu:203-223 */
int kt_transform_maps(kt_ctx* ctx, const float* vmap_src, const float* nmap_src, int cols, int rows,
                      const kt_mat33* Rmat, const float tvec[3], float* vmap_dst, float* nmap_dst);
/* resizeVMap / resizeNMap  internal.h:453,460 / maps.cu:279-308; out is (in_cols/2) x (in_rows/2) */
int kt_resize_vmap(kt_ctx* ctx, const float* in, int in_cols, int in_rows, float* out);
int kt_resize_nmap(kt_ctx* ctx, const float* in, int in_cols, int in_rows, float* out);
/* generateImage  internal.h:435 / image_generator.cu:56-179: shaded + colour views of a predicted map (vmap_curr_color = the uchar4
 * raycast colour output); dst / dst_color are rgb24 [rows][cols][3].  light_number <= 1 (LightSource holds one position). */
int kt_generate_image(kt_ctx* ctx, const float* vmap, const float* nmap, const uint8_t* vmap_curr_color, int cols, int rows,
                      const float light_pos[3], int light_number, uint8_t* dst_rgb24, uint8_t* dst_color_rgb24);
/* generateDepth  internal.h:442 / image_generator.cu:181-219: depth image (mm) of a predicted map seen from pose (R_inv, t) */
int kt_generate_depth(kt_ctx* ctx, const kt_mat33* R_inv, const float t[3], const float* vmap, const float* nmap, int cols, int rows,
                      uint16_t* dst);
/* shortDepthToMetres  internal.h:313 / bilateral_pyrdown.cu:404-411 */
int kt_depth_to_metres(kt_ctx* ctx, const uint16_t* src, float* dst, int cols, int rows, int cutoff);
/* imageBGRToIntensity  internal.h:315 / bilateral_pyrdown.cu:413-420; src = rgb24 */
int kt_bgr_to_intensity(kt_ctx* ctx, const uint8_t* src_rgb24, uint8_t* dst, int cols, int rows);
/* pyrDownGaussF  internal.h:309 / bilateral_pyrdown.cu:356-377 */
int kt_pyr_down_gauss_f32(kt_ctx* ctx, const float* src, int scols, int srows, float* dst);
/* pyrDownUcharGauss  internal.h:311 / bilateral_pyrdown.cu:379-402 */
int kt_pyr_down_gauss_u8(kt_ctx* ctx, const uint8_t* src, int scols, int srows, uint8_t* dst);
/* computeDerivativeImages  internal.h:301 / bilateral_pyrdown.cu:300-330 */
int kt_derivative_images(kt_ctx* ctx, const uint8_t* src, int cols, int rows, int16_t* dx, int16_t* dy);
/* projectToPointCloud  internal.h:317-320 / maps.cu:329-344; cloud = float[rows][cols][3]; intrinsics of level 0 */
int kt_project_to_cloud(kt_ctx* ctx, const float* depth, int cols, int rows, float* cloud_xyz,
                        double fx, double fy, double cx, double cy, int level);

/* Fused pyramid build (no single reference counterpart): pyrDown x3 + createVMap x4 + createNMap x4 in one launch,
 * bit-identical to the separate calls (KintinuousTracker.cpp:469-478).  depth0 = bilateral-filtered level 0. */
int kt_build_pyramid(kt_ctx* ctx, const kt_intr* intr, const uint16_t* depth0, int cols, int rows,
                     uint16_t* const depths_out[3], float* const vmaps[4], float* const nmaps[4]);

/* ---- tracking reductions ---- */
/* icpStep  internal.h:485-502 / reduce.cu:347-419.  A_host[36] row-major symmetric, b_host[6], residual_host[2]
 * = {sum residual^2, inlier count}.  The reference's `sum`/`out` scratch arrays live in the context. */
int kt_icp_step(kt_ctx* ctx, const kt_mat33* Rcurr, const float tcurr[3], const float* vmap_curr, const float* nmap_curr,
                const kt_mat33* Rprev_inv, const float tprev[3], const kt_intr* intr,
                const float* vmap_g_prev, const float* nmap_g_prev, int cols, int rows,
                float dist_thres, float angle_thres, float* A_host, float* b_host, float* residual_host);
/* ICPOdometry::getIncrementalTransformation as one call (frontend/ICPOdometry.cpp:68-186; SURVEY 8(b) export list): pose in, pose out.
 * maps[l] = level l of the four pyramids (3 * (rows >> l) planes of (cols >> l) floats; a level with iterations[l] == 0 may be null),
 * intr = level-0 intrinsics (level l uses intr / 2^l, internal.h:255-259), iterations[l] = Gauss-Newton iterations at level l, run
 * from level 3 down to 0 (the reference: {10, 5, 4, 0}, fast odometry {0, 10, 5, 0}, ICPOdometry.cpp:44-55).  Every iteration is a
 * device launch whose epilogue solves the 6x6 system in double (Eigen's pivoted LDLT restated), applies cv::Rodrigues and the
 * SE(3) update (:127-178) and leaves the pose on the device for the next one: no host round trip until the final read-back.
 * A_last_host[36] (may be null) = the last iteration's A, row-major symmetric (the reference keeps it as lastA for getCovariance);
 * residual_host[2] (may be null) = that iteration's {sum residual^2, inlier count}.  Poses are bit-identical to iterating kt_icp_step
 * + kt_host_ldlt_solve6 + kt_host_pose_update on the host. */
int kt_icp_track(kt_ctx* ctx, const float* const vmaps_curr[4], const float* const nmaps_curr[4], const float* const vmaps_g_prev[4],
                 const float* const nmaps_g_prev[4], int cols, int rows, const kt_intr* intr, const kt_mat33* Rprev, const float tprev[3],
                 const int iterations[4], float dist_thres, float angle_thres, kt_mat33* Rcurr_host, float tcurr_host[3],
                 float A_last_host[36], float residual_host[2]);
/* computeRgbResidual  internal.h:519-534 / reduce.cu:798-864 */
int kt_rgb_residual(kt_ctx* ctx, float min_scale, const int16_t* dIdx, const int16_t* dIdy,
                    const float* last_depth, const float* next_depth, const uint8_t* last_image, const uint8_t* next_image,
                    int cols, int rows, kt_dataterm* corres_img, float max_depth_delta, const float kt[3],
                    const kt_mat33* krkinv, int* sigma_sum_host, int* count_host);
/* rgbStep  internal.h:504-517 / reduce.cu:555-607 */
int kt_rgb_step(kt_ctx* ctx, const kt_dataterm* corres_img, float sigma, const float* cloud_xyz, float fx, float fy,
                const int16_t* dIdx, const int16_t* dIdy, float sobel_scale, int cols, int rows,
                float* A_host, float* b_host);

/* ---- volume kernels ---- */
/* initVolume / initColorVolume  internal.h:353,417 / tsdf_volume.cu:468-479, 76-87 */
int kt_init_volume(kt_ctx* ctx, int16_t* volume, int N);
int kt_init_color_volume(kt_ctx* ctx, uint8_t* color_volume, int N);
/* integrateTsdfVolume  internal.h:404-409 / tsdf_volume.cu:642-674.  colors = rgb24, nmap_curr = level-0 normal map.
 * Precondition on the volume pair: a state these kernels can leave behind, i.e. grown from kt_init_volume / kt_init_color_volume by
 * integrate and the clears -- weight bytes <= 128 (MAX_WEIGHT).  Any tsdf word and any colour is followed bit for bit
 * (tests/test_gpu_sweep.py::test_random_state_integrate_hip); a foreign volume with a weight byte above 128 keeps that weight where the
 * reference would clamp it to 128 (tests/tools/state_probe.py). */
int kt_integrate_tsdf(kt_ctx* ctx, const uint16_t* depth_raw, int cols, int rows, const kt_intr* intr,
                      const float volume_size[3], const kt_mat33* Rcurr_inv, const float tcurr[3], float tranc_dist,
                      int16_t* volume, float* depth_raw_scaled, const int voxel_wrap[3], uint8_t* color_volume,
                      const uint8_t* colors_rgb24, const float* nmap_curr, int angle_color, int N);
/* raycast  internal.h:429-431 / ray_caster.cu:433-471.  vmap_curr_color = uint8[rows][cols][4] */
int kt_raycast(kt_ctx* ctx, const kt_intr* intr, const kt_mat33* Rcurr, const float tcurr[3], float tranc_dist,
               const float volume_size[3], const int16_t* volume, float* vmap, float* nmap, int cols, int rows,
               const int voxel_wrap[3], uint8_t* vmap_curr_color, const uint8_t* color_volume, int N);
/* clearVolume{X,Y,Z}{,Back}{,c}  internal.h:355-389 / tsdf_volume.cu:117-448.
 * axis 0/1/2 = X/Y/Z, back = the ...Back variants, elem_size 2 = tsdf (short), 4 = colour (uchar4, the ...c variants) */
int kt_clear_volume(kt_ctx* ctx, void* volume, int elem_size, int N, int axis, int back,
                    int current_voxel_wrap, int delta_voxel_wrap);
/* extractCloudSlice  internal.h:463-476 / extract.cu:325-419.  Output order is unspecified (as in the reference). */
int kt_extract_cloud_slice(kt_ctx* ctx, const int16_t* volume, const float volume_size[3], kt_point_xyzrgb* output,
                           size_t output_capacity, const int voxel_wrap[3], const uint8_t* color_volume,
                           int minX, int maxX, int minY, int maxY, int minZ, int maxZ, int subsample,
                           const int real_voxel_wrap[3], int N, size_t* count_host);
/* Marching cubes of the volume over a box of CELLS [lo, hi) per axis, 0 <= lo <= hi <= N - 1 (no reference counterpart: its -m
 * triangulates the processed cloud with PCL's greedy projection, backend/MeshGenerator.cpp; kt_mesh.hip).  Cell (x, y, z) has the
 * corners (x..x+1, y..y+1, z..z+1) in logical coordinates, stored under voxel_wrap as in kt_extract_cloud_slice.  A voxel is valid
 * when its weight != 0 and its tsdf F != 1 (the extraction's rule), a cell is meshed when its 8 corners are, a corner is inside when
 * F < 0.  One vertex per crossed edge next to a meshed cell of the box, at the position and with the colour word kt_extract_cloud_slice
 * gives the point of that (voxel, axis) pair (real_voxel_wrap included): on an edge whose tsdf changes sign strictly the vertex IS that
 * point, bit for bit.  Vertices in (owner voxel z, y, x, axis) order, the owner being the edge's lower end; triangles (uint32[3] vertex
 * indices, normal (v1 - v0) x (v2 - v0) pointing to F > 0) by cell (z, y, x), then case-table order (kt_mc_table.hpp, generated by
 * kintinuous_amd/mc_table.py: no cracks between cells).  The output is deterministic.  vertices / triangles: device (or pinned host)
 * buffers of vertex_capacity / triangle_capacity entries.  Synchronises; *n_vertices / *n_triangles = the mesh's true sizes.  If
 * either exceeds its capacity, or the mesh has more than 2^29 vertices, NOTHING is written and KT_ERR_CAPACITY is returned. */
int kt_extract_mesh(kt_ctx* ctx, const int16_t* volume, const float volume_size[3], const int voxel_wrap[3], const uint8_t* color_volume,
                    const int lo[3], const int hi[3], const int real_voxel_wrap[3], int N, kt_mesh_vertex* vertices,
                    size_t vertex_capacity, uint32_t* triangles, size_t triangle_capacity, size_t* n_vertices, size_t* n_triangles);
/* kt_extract_mesh, and beside every vertex the key of the voxel edge it lies on:
 *   (gz + 2^19) << 42 | (gy + 2^19) << 22 | (gx + 2^19) << 2 | axis,  g = the owner voxel (logical) + real_voxel_wrap, axis 0 (x), 1 or 2;
 * the top two bits are zero.  Two calls that emit a vertex on the same global edge -- two slabs of the mesh stage on the plane between
 * them -- give it the same key (kt_mesh_weld merges them); the position alone does not name the edge, since a vertex at F == 0 sits
 * on a voxel centre and fits three axes.  The keys of one call are strictly increasing.  keys: a device (or pinned host) buffer of
 * vertex_capacity entries, written exactly where vertices are (nothing on KT_ERR_CAPACITY).  Vertices and triangles are
 * kt_extract_mesh's, byte for byte.  KT_ERR_ARG before any work when a global voxel of the box's voxels [lo, hi] lies outside
 * [-2^19, 2^19). */
int kt_extract_mesh_keyed(kt_ctx* ctx, const int16_t* volume, const float volume_size[3], const int voxel_wrap[3], const uint8_t* color_volume,
                          const int lo[3], const int hi[3], const int real_voxel_wrap[3], int N, kt_mesh_vertex* vertices,
                          size_t vertex_capacity, uint32_t* triangles, size_t triangle_capacity, uint64_t* keys, size_t* n_vertices,
                          size_t* n_triangles);

/* Welds the vertices of a mesh that share an edge key (kt_mesh_weld.hip; restated by kintinuous_amd/mesh_weld_ref.py, which the device
 * equals on every byte).  Input: n vertices and n keys, m triangles (uint32[3] indices below n), and the span table of
 * kt_deform_apply_mesh (span_first: n_spans + 1 host entries from 0 to n, non-decreasing; span_time: n_spans host entries).
 *   - The occurrences of a key are taken in index order.  An occurrence starts a new group when it is the first of its key, or when its
 *     span's time and the previous occurrence's span's time differ by more than max_gap (the larger minus the smaller; UINT64_MAX: no
 *     gate).  The gate is the caller's: keys are global voxels, so a place the camera returns to much later carries the same keys for
 *     what, under drift, is another pass over the surface, which a deformation must stay free to move.
 *   - The representative of a vertex is the first vertex of its group.  Kept vertices are the representatives, in input order, their
 *     16 bytes and their keys untouched: a welded vertex keeps the EARLIER slab's position, colour and span (that plane had its full
 *     fusion history when the earlier slab left).
 *   - Every triangle index becomes the new index of its vertex's representative; triangles are neither dropped nor reordered (a
 *     triangle of kt_extract_mesh has three distinct keys and cannot collapse).
 *   - span_first_out[s] (n_spans + 1 host entries) = the number of kept vertices below span_first[s]: the welded mesh and this table
 *     go straight into kt_deform_apply_mesh.
 * kt_mesh_weld_device: device arrays; the triangles are remapped IN PLACE, the kept vertices and keys go to vertices_out_dev /
 * keys_out_dev (vertex_capacity entries each, not the input arrays); everything is enqueued on the object's stream and the host waits
 * once, for *n_out.  kt_mesh_weld: the same on host arrays (upload, weld, download; triangles in place).
 * KT_ERR_ARG with nothing written: a span table that does not start at 0, decreases or does not end at n; null pointers with n > 0;
 * vertices not 16-byte aligned; n > 2^29; a key with a top bit set.  KT_ERR_CAPACITY with nothing written and the triangles intact
 * when *n_out > vertex_capacity (*n_out is reported).  n = 0: KT_OK.  What is left after the weld: a crack where the tsdf's sign change
 * sits on a different edge at the two times, and the one-cell gap of kt_tracker_enable_mesh_stage.
 * The object owns its workspace (about 24 bytes per vertex and the sort's), which grows with the calls; hip_stream null: the context's. */
typedef struct kt_mesh_welder kt_mesh_welder;
int kt_mesh_weld_create(kt_ctx* ctx, void* hip_stream, kt_mesh_welder** out);
int kt_mesh_weld_destroy(kt_mesh_welder* w);
int kt_mesh_weld_device(kt_mesh_welder* w, const kt_mesh_vertex* vertices_dev, const uint64_t* keys_dev, size_t n, uint32_t* triangles_dev, size_t m,
                        const size_t* span_first, const uint64_t* span_time, int n_spans, uint64_t max_gap, kt_mesh_vertex* vertices_out_dev,
                        uint64_t* keys_out_dev, size_t vertex_capacity, size_t* span_first_out, size_t* n_out);
int kt_mesh_weld(kt_mesh_welder* w, const kt_mesh_vertex* vertices, const uint64_t* keys, size_t n, uint32_t* triangles, size_t m,
                 const size_t* span_first, const uint64_t* span_time, int n_spans, uint64_t max_gap, kt_mesh_vertex* vertices_out,
                 uint64_t* keys_out, size_t vertex_capacity, size_t* span_first_out, size_t* n_out);

/* Coarsens a mesh by vertex clustering (kt_mesh_simplify.hip; restated by kintinuous_amd/mesh_simplify_ref.py, which the device equals
 * on every byte).  Input: n vertices, m triangles (uint32[3] indices below n), the span table of kt_mesh_weld (span_first only) and
 * cell, the edge of the clustering cells in metres.
 *   - inv = 1 / (double)cell once; per axis c = floor((double)x * inv).  A vertex is valid when x, y, z are finite, |coordinate| < 8192
 *     and every c lies in [-2^19, 2^19); key = (cz + 2^19) << 40 | (cy + 2^19) << 20 | (cx + 2^19).
 *   - The occurrences of a key are taken in index order.  An occurrence starts a new cluster when it is the first of its key or when
 *     its span differs from the previous occurrence's: a cluster is one cell of one span.  Output vertices are one per cluster, in the
 *     order of the clusters' first vertices; span_first_out[s] = the number of output vertices whose cluster starts below span_first[s],
 *     so the result and this table go straight into kt_deform_apply_mesh.
 *   - The output vertex, in integers: per member and axis q = rint((double)x * 2^20) (ties to even), S = the sum, k = the member count,
 *     mean = floor((2 S + k) / (2 k)), the coordinate (float)((double)mean * 2^-20); each of the four bytes of the colour word by the
 *     same rule.  A cluster of one member keeps its 16 bytes: a cell below every vertex spacing returns the input.
 *   - Every triangle index becomes its vertex's cluster; a triangle with two equal indices is dropped; the others keep their order
 *     and orientation (duplicates among them stay).
 * kt_mesh_simplify_device: device arrays; vertices and triangles go to vertices_out_dev (vertex_capacity entries) and
 * triangles_out_dev (triangle_capacity triangles), neither an input array; everything is enqueued on the object's stream and the host
 * waits once, for *n_out and *m_out.  kt_mesh_simplify: the same on host arrays (upload, simplify, download).
 * KT_ERR_ARG with nothing written: cell not finite or <= 0; a bad span table; null pointers with n > 0; vertices not 16-byte aligned;
 * an output array that is an input array; n > 2^29 or m > 2^31; any invalid vertex.  KT_ERR_CAPACITY with nothing written when
 * *n_out > vertex_capacity or *m_out > triangle_capacity (both true counts are reported).  n = 0: KT_OK.
 * The object owns its workspace (about 100 bytes per vertex and the sort's), which grows with the calls; hip_stream null: the context's. */
typedef struct kt_mesh_simplifier kt_mesh_simplifier;
int kt_mesh_simplify_create(kt_ctx* ctx, void* hip_stream, kt_mesh_simplifier** out);
int kt_mesh_simplify_destroy(kt_mesh_simplifier* w);
int kt_mesh_simplify_device(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m,
                            const size_t* span_first, int n_spans, float cell, kt_mesh_vertex* vertices_out_dev, size_t vertex_capacity,
                            uint32_t* triangles_out_dev, size_t triangle_capacity, size_t* span_first_out, size_t* n_out, size_t* m_out);
int kt_mesh_simplify(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m,
                     const size_t* span_first, int n_spans, float cell, kt_mesh_vertex* vertices_out, size_t vertex_capacity,
                     uint32_t* triangles_out, size_t triangle_capacity, size_t* span_first_out, size_t* n_out, size_t* m_out);

/* The quadric form of the simplification, on the same object (kt_mesh_simplify.hip; Lindstrom's out-of-core simplification, 2000;
 * restated by mesh_simplify_ref.simplify_quadric, which the device equals on every byte).  Clusters, heads, output order,
 * span_first_out, colour bytes, the triangle map, the dropped triangles and the rule that a cluster of one member keeps its 16 bytes are
 * kt_mesh_simplify's; only the xyz of a cluster with more than one member can differ: it is the minimiser of the summed plane quadrics of
 * the triangles that touch the cluster, regularised towards the mean by `bias`, where that minimiser lies in the cluster's own cell.
 *   - Per input triangle: an index >= n is an error; a triangle with two equal indices contributes nothing; otherwise its indices are
 *     rotated so that the smallest comes first (v0, v1, v2, orientation kept): the result depends on neither the rotation of a triangle
 *     nor the order of the list.
 *   - In double, every operation rounded once: e1 = (double)v1 - (double)v0, e2 = (double)v2 - (double)v0 per axis; c = e1 x e2 in
 *     kt_mesh_normals' order (c_x = e1y e2z - e1z e2y, ...); len = sqrt((cx cx + cy cy) + cz cz); c == (0, 0, 0) contributes nothing;
 *     nh = c / len per axis.
 *   - For every DISTINCT cluster among the clusters of v0, v1, v2, once per cluster: k_a = floor((double)x_a * inv) of the triangle's
 *     vertex in that cluster (the cluster's cell), o_a = ((double)k_a + 0.5) * (double)cell, r = (double)v0 - o,
 *     d = (nhx rx + nhy ry) + nhz rz; the nine terms c_i * nh_j for i <= j (xx, xy, xz, yy, yz, zz) and c_i * d (x, y, z).  A term that
 *     is not |term| < 1 is an error; q = (int64)rint(term * 2^32), ties to even, is added to the cluster's nine int64 sums.  m <= 2^29,
 *     so |S| <= 2^61, and integer addition commutes: scheduling cannot change a bit.
 *   - Per cluster with more than one member: mean_q the integer mean of kt_mesh_simplify per axis, m_a = (double)mean_q_a * 2^-20 - o_a,
 *     t = ((double)Sxx + (double)Syy) + (double)Szz, lam = (double)bias * t, M = (double)S_A + lam I, r_a = (double)S_b_a + lam * m_a;
 *     c00 = M11 M22 - M12 M12, c01 = M02 M12 - M01 M22, c02 = M01 M12 - M02 M11, c11 = M00 M22 - M02 M02, c12 = M01 M02 - M00 M12,
 *     c22 = M00 M11 - M01 M01, det = (M00 c00 + M01 c01) + M02 c02, x0 = ((c00 r0 + c01 r1) + c02 r2) / det,
 *     x1 = ((c01 r0 + c11 r1) + c12 r2) / det, x2 = ((c02 r0 + c12 r1) + c22 r2) / det, out_a = (float)(o_a + x_a).  The cluster is
 *     PLACED when t > 0, det > 0, every out_a is finite and floor((double)out_a * inv) == k_a on all three axes; otherwise it keeps the
 *     mean's bytes.  *n_placed counts the placed clusters.
 * bias is finite and in [2^-20, 1] (the driver's default is 2^-6): a small one keeps edges and corners sharper, a large one keeps the
 * vertex nearer the mean where the planes leave it free.  On a smooth noisy surface the minimiser wanders tangentially and is no better
 * than the mean.  Rims are not held by boundary quadrics, flipped triangles are not looked for, duplicate survivors stay.
 * KT_ERR_ARG with nothing written: everything of kt_mesh_simplify; a bias outside its range; m > 2^29; a triangle index >= n; a term of
 * 1 or more (a triangle of about 1 m^2).  KT_ERR_CAPACITY as kt_mesh_simplify.  The nine sums (72 bytes per vertex) are a buffer of their
 * own, taken on the first quadric call: an object that only runs kt_mesh_simplify never holds it.  The two forms may be called in any
 * order on one object. */
int kt_mesh_simplify_quadric_device(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m,
                                    const size_t* span_first, int n_spans, float cell, float bias, kt_mesh_vertex* vertices_out_dev,
                                    size_t vertex_capacity, uint32_t* triangles_out_dev, size_t triangle_capacity, size_t* span_first_out,
                                    size_t* n_out, size_t* m_out, size_t* n_placed);
int kt_mesh_simplify_quadric(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m,
                             const size_t* span_first, int n_spans, float cell, float bias, kt_mesh_vertex* vertices_out, size_t vertex_capacity,
                             uint32_t* triangles_out, size_t triangle_capacity, size_t* span_first_out, size_t* n_out, size_t* m_out,
                             size_t* n_placed);

/* Vertex normals of a mesh from its own triangles (kt_mesh_normals.hip; restated by kintinuous_amd/mesh_normals_ref.py, which the device
 * equals on every byte, on every call).  Input: n vertices and m triangles (uint32[3]).  Output: n normals and *n_zero, the number of
 * vertices whose normal is (0, 0, 0).
 *   - Per triangle (i0, i1, i2): an index >= n is an error.  A triangle with two equal indices contributes nothing.  Otherwise each of
 *     its three vertices must be valid: x, y, z finite and |coordinate| < 8192 (kt_mesh_simplify's rule).
 *   - In double, every operation rounded once and none contracted: e1 = (double)v1 - (double)v0 and e2 = (double)v2 - (double)v0 per
 *     axis, c = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), each component two products and one subtraction, in that
 *     order.  This is the (v1 - v0) x (v2 - v0) that points to F > 0 on a mesh of kt_extract_mesh; its length is twice the triangle's
 *     area, so the sum below is area-weighted and the slivers of marching cubes do not steer the normal.
 *   - A triangle with any |c component| >= 1.0 (1 m^2) is an error.  q = (int64)rint(c * 2^32) per component, ties to even; the same q
 *     is added to the sums of i0, i1 and i2.
 *   - Per vertex, S = the three int64 sums over its triangles.  All three zero (an isolated vertex, exact cancellation, slivers only):
 *     the normal is (0, 0, 0) and the vertex is counted in *n_zero.  Otherwise d = (double)S per axis,
 *     len = sqrt((dx dx + dy dy) + dz dz), normal = (float)(d / len) per axis.  A vertex that no triangle references is not validated.
 *   - |q| <= 2^32, a vertex takes at most one q per triangle and m <= 2^29, so |S| <= 2^61: the sums cannot overflow, and integer
 *     addition commutes, so the result does not depend on scheduling or on the order of the triangles.
 * kt_mesh_normals_device: device arrays; everything is enqueued on the object's stream and the host waits once, for the status and
 * *n_zero.  kt_mesh_normals: the same on host arrays (upload, compute, download).
 * KT_ERR_ARG with nothing written to the output: an index out of range; an invalid referenced vertex; a triangle over the bound; null
 * pointers with n > 0; vertices not 16-byte aligned; the output overlapping an input; n > 2^29 or m > 2^29 (refused before any
 * allocation or launch).  n = 0 or m = 0: KT_OK and all normals zero (with n = 0 the triangles are not looked at).
 * The object owns its workspace (24 bytes per vertex), which grows with the calls; hip_stream null: the context's. */
typedef struct { float nx, ny, nz; } kt_mesh_normal;
typedef struct kt_mesh_normal_pass kt_mesh_normal_pass;
int kt_mesh_normals_create(kt_ctx* ctx, void* hip_stream, kt_mesh_normal_pass** out);
int kt_mesh_normals_destroy(kt_mesh_normal_pass* w);
int kt_mesh_normals_device(kt_mesh_normal_pass* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m,
                           kt_mesh_normal* normals_out_dev, size_t* n_zero);
int kt_mesh_normals(kt_mesh_normal_pass* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m,
                    kt_mesh_normal* normals_out, size_t* n_zero);

/* Drops the small disconnected pieces of a mesh (kt_mesh_components.hip; restated by kintinuous_amd/mesh_components_ref.py, which the
 * device equals on every byte, on every call).  Input: n vertices, m triangles (uint32[3]), the span table of kt_mesh_weld (span_first
 * only) and min_triangles.
 *   - Two vertices are joined when one triangle holds both: every triangle joins its three indices, one with repeated indices included.
 *     Position plays no part: two vertices with equal coordinates and different indices are NOT joined (the unwelded slab seam: run
 *     kt_mesh_weld first).  An index >= n is an error.
 *   - label[v] = the smallest vertex index of v's component (the components of that relation's transitive closure).
 *   - The size of a component = the number of triangles whose FIRST index carries its label; duplicate triangles count each time; a
 *     vertex that no triangle references is a component of size 0.
 *   - A component is kept when size >= min_triangles.  0 keeps everything (the output is the input byte for byte, unreferenced vertices
 *     included); 1 drops exactly the unreferenced vertices.
 *   - Output vertices: those of kept components, in input order, their 16 bytes untouched.  Output triangles: those of kept components,
 *     in input order, orientation kept, every index replaced by the number of kept vertices below it.
 *   - span_first_out[s] (n_spans + 1 host entries) = the number of kept vertices below span_first[s]: the result and this table go
 *     straight into kt_deform_apply_mesh, kt_mesh_simplify and kt_mesh_normals.
 *   - labels_out (n entries, may be null) receives label[v] for every INPUT vertex, dropped ones too.
 *   - stats: all components (those of size 0 included), the kept ones, and the triangles of the largest.
 * kt_mesh_components_device: device arrays; everything is enqueued on the object's stream and the host waits once, for the status, the
 * counts and the stats.  The result depends on neither the scheduling nor the order of the triangles (kt_unionfind.hpp: the last root
 * of a component is its smallest index under every interleaving; the sizes are integer sums).  kt_mesh_components: the same on host
 * arrays (upload, run, download).
 * KT_ERR_ARG with nothing written to any output: an index out of range; a bad span table; null pointers with n > 0; vertices not 16-byte
 * aligned; an output that is or overlaps an input or another output; n > 2^29 or m > 2^29 (refused before any allocation or launch).
 * KT_ERR_CAPACITY with nothing written when *n_out > vertex_capacity or *m_out > triangle_capacity (both true counts are reported).
 * n = 0: KT_OK and zeros (the triangles are not looked at).  m = 0 with n > 0: n components of size 0.
 * The object owns its workspace (16 bytes per vertex, and 4 bytes per 256 vertices and per 256 triangles), which grows with the calls;
 * hip_stream null: the context's. */
typedef struct kt_mesh_component_pass kt_mesh_component_pass;
typedef struct { uint64_t components, kept_components, largest; } kt_mesh_component_stats;   /* largest: triangles of the biggest component */
int kt_mesh_components_create(kt_ctx* ctx, void* hip_stream, kt_mesh_component_pass** out);
int kt_mesh_components_destroy(kt_mesh_component_pass* w);
int kt_mesh_components_device(kt_mesh_component_pass* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m,
                              const size_t* span_first, int n_spans, uint32_t min_triangles, kt_mesh_vertex* vertices_out_dev, size_t vertex_capacity,
                              uint32_t* triangles_out_dev, size_t triangle_capacity, uint32_t* labels_out_dev, size_t* span_first_out, size_t* n_out,
                              size_t* m_out, kt_mesh_component_stats* stats);
int kt_mesh_components(kt_mesh_component_pass* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m,
                       const size_t* span_first, int n_spans, uint32_t min_triangles, kt_mesh_vertex* vertices_out, size_t vertex_capacity,
                       uint32_t* triangles_out, size_t triangle_capacity, uint32_t* labels_out, size_t* span_first_out, size_t* n_out, size_t* m_out,
                       kt_mesh_component_stats* stats);

/* Reports the open boundaries of a mesh and fills its small holes (kt_mesh_holes.hip; restated by kintinuous_amd/mesh_holes_ref.py, which
 * the device equals on every byte, on every call).  Input: n vertices, m triangles (uint32[3]), the span table of kt_mesh_weld (span_first
 * only) and max_edges in [0, 256].
 *   - Triangle t, corner k gives half-edge h = 3 t + k from a = tri[t][k] to b = tri[t][(k + 1) % 3].  A triangle with two equal indices
 *     is degenerate: it has no half-edges, it is counted, and it is copied to the output like any other.  An index >= n is an error.
 *   - An undirected edge {a, b} with f half-edges min -> max and r the other way is interior when f == r == 1, boundary when f + r == 1,
 *     and non-manifold otherwise: counted once per edge, both end vertices BLOCKED.
 *   - out[v] and in[v] count the boundary half-edges that leave and enter v.  A vertex with in + out > 0 and not in == out == 1 is COMPLEX.
 *   - The boundary half-edges join their two vertices into boundary components; the label is the component's smallest vertex index.  A
 *     component none of whose vertices is COMPLEX or BLOCKED is a simple loop: one cycle, its length L its vertex count.  Any other is an
 *     open component: counted, never filled.
 *   - A simple loop is filled when 3 <= L <= max_edges and every vertex of it is valid (x, y, z finite and |coordinate| < 8192,
 *     kt_mesh_simplify's rule).  max_edges of 0, 1 or 2 fills nothing: the call only reports.
 *   - The centre vertex of a filled loop, per coordinate: q = rint((double)x * 2^32) as int64, S = the sum of q over the loop (exact in
 *     double: |S| < 2^53), c = (float)((double)S / (double)L * 2^-32).  Each of the four bytes of rgb is (2 * sum + L) / (2 L) in integers.
 *   - One fill triangle (b, a, centre) per boundary half-edge a -> b of a filled loop: every edge of the fan is interior afterwards and
 *     the orientation agrees with the neighbour's.
 *   - Output vertices stay in their spans: span s holds its input vertices in input order, then the centres of the filled loops whose
 *     label lies in span s, ascending by label.  span_first_out[s] (n_spans + 1 host entries) is the new first vertex per span: the result
 *     and this table go straight into kt_mesh_components, kt_mesh_simplify, kt_mesh_normals and kt_deform_apply_mesh.
 *   - Output triangles: the m input triangles in input order through the index map, then the fill triangles ascending by h.
 *   - loop_out (n entries, may be null): the label for a vertex of a simple loop, 0xfffffffe for a boundary vertex of an open component,
 *     0xffffffff for any other vertex.
 *   - stats: the boundary edges, the non-manifold edges, the degenerate triangles, the simple loops, the open components, the filled
 *     loops, the edges of the longest simple loop, and the vertices and triangles added.
 * The long one-cell gap between two slabs is two long rims: it is reported and not closed.  A small open patch's own rim is a small loop
 * and gets capped: run kt_mesh_components first.
 * kt_mesh_holes_device: device arrays; everything is enqueued on the object's stream and the host waits once.  The result depends on
 * neither the scheduling nor, for the vertices, loop_out and the set of triangles, the order of the triangles (kt_unionfind.hpp: the last
 * root of a component is its smallest index under every interleaving; every count and sum is an integer sum).  kt_mesh_holes: the same on
 * host arrays (upload, run, download).
 * KT_ERR_ARG with nothing written to any output: an index out of range; a bad span table; null pointers with n > 0; vertices not 16-byte
 * aligned; an output that is or overlaps an input or another output; n > 2^29 or m > 2^29 (refused before any allocation or launch);
 * max_edges > 256.
 * KT_ERR_CAPACITY with nothing written when *n_out > vertex_capacity or *m_out > triangle_capacity (both true counts are reported).  No
 * call gives more than n + n / 3 vertices and m + min(n, 3 m) triangles.
 * n = 0: KT_OK and zeros (the triangles are not looked at).  m = 0 with n > 0: the output is the input.
 * The object owns its workspace (32 bytes per vertex, 40 per three vertices, 24 per half-edge and the sort's own), which grows with the
 * calls; hip_stream null: the context's. */
typedef struct kt_mesh_hole_pass kt_mesh_hole_pass;
typedef struct {
    uint64_t boundary_edges, nonmanifold_edges, degenerate_triangles, loops, open_components, filled;
    uint64_t longest;   /* edges of the longest simple loop */
    uint64_t new_vertices, new_triangles;
} kt_mesh_hole_stats;
int kt_mesh_holes_create(kt_ctx* ctx, void* hip_stream, kt_mesh_hole_pass** out);
int kt_mesh_holes_destroy(kt_mesh_hole_pass* w);
int kt_mesh_holes_device(kt_mesh_hole_pass* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m,
                         const size_t* span_first, int n_spans, uint32_t max_edges, kt_mesh_vertex* vertices_out_dev, size_t vertex_capacity,
                         uint32_t* triangles_out_dev, size_t triangle_capacity, uint32_t* loop_out_dev, size_t* span_first_out, size_t* n_out,
                         size_t* m_out, kt_mesh_hole_stats* stats);
int kt_mesh_holes(kt_mesh_hole_pass* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, const size_t* span_first,
                  int n_spans, uint32_t max_edges, kt_mesh_vertex* vertices_out, size_t vertex_capacity, uint32_t* triangles_out,
                  size_t triangle_capacity, uint32_t* loop_out, size_t* span_first_out, size_t* n_out, size_t* m_out, kt_mesh_hole_stats* stats);

/* Smooths a mesh with Taubin's lambda|mu filter (kt_mesh_smooth.hip; restated by kintinuous_amd/mesh_smooth_ref.py, which the device
 * equals on every byte, on every call).  Input: n vertices, m triangles (uint32[3]), steps in [0, 64], lambda in (0, 1], mu in [-1.1, 1]
 * (compared as floats; mu = lambda, plain Laplacian smoothing, is allowed) and mode 0 or 1.  Output: n vertices in the same order with
 * the same rgb; no vertex is added, dropped or renumbered, so the triangles and any span table hold for the output as they are.
 *   - Half-edges as for kt_mesh_holes: a triangle with two equal indices has none.  An index >= n is an error.
 *   - An undirected edge with exactly one half-edge each way is interior; any other (boundary or non-manifold) is rim.  A vertex is rim
 *     when it is an end of a rim edge.  An undirected edge counts once, however many triangles hold it: uniform umbrella weights.
 *   - Neighbours: an interior vertex has the other ends of all its edges.  A rim vertex has none with mode 0 (the rims are pinned) and
 *     the other ends of its rim edges with mode 1 (it moves along the rim).  d = the number of neighbours; d > 65535 is an error; a
 *     vertex with d = 0 does not move.
 *   - A vertex that is an end of a half-edge must be valid: x, y, z finite and |coordinate| < 8192 (kt_mesh_simplify's rule).  Any other
 *     vertex is not validated.
 *   - State, per vertex and coordinate: the int64 q = rint((double)x * 2^32), so |q| < 2^45.
 *   - One half-step with the factor f = (double)lambda or (double)mu, for every vertex with d > 0: S = the int64 sum of the neighbours' q
 *     from BEFORE the half-step, D = S - d q (exact, |D| < 2^62), q' = q + (int64)rint(f * ((double)D / (double)d)).  The conversion of D,
 *     the division and the product are rounded once each, rint rounds ties to even, nothing is contracted.  |q'| >= 2^45 is an error.
 *   - One step is the lambda half-step followed by the mu half-step.
 *   - Output: a vertex with d = 0, and every vertex when steps = 0, is copied byte for byte (float -> q -> float is not the identity for
 *     small |x|).  Any other vertex gets x = (float)((double)q * 2^-32) per coordinate, its rgb copied.
 *   - stats: the rim vertices, the vertices with d > 0 when steps > 0 (0 otherwise), the undirected edges.
 * kt_mesh_smooth_device: device arrays; everything is enqueued on the object's stream and the host waits once.  Integer addition
 * commutes and a half-step reads only the state before it, so the result depends on neither the scheduling nor the order of the
 * triangles.  kt_mesh_smooth: the same on host arrays (upload, run, download).
 * KT_ERR_ARG with nothing written to the output or the stats: an index out of range; an invalid referenced vertex; a valence over the
 * bound; a coordinate that left the range; null pointers with n > 0; vertices not 16-byte aligned; the output being or overlapping an
 * input; n > 2^29 or m > 2^29 (refused before any allocation or launch); steps, lambda, mu (a NaN included) or mode out of range.
 * n = 0: KT_OK, nothing done (the triangles are not looked at).  m = 0 with n > 0: the output is the input.
 * The object owns its workspace (64 bytes per vertex, 29 per half-edge and the sort's own), which grows with the calls; hip_stream null:
 * the context's. */
typedef struct kt_mesh_smooth_pass kt_mesh_smooth_pass;
typedef struct { uint64_t rim_vertices, moved_vertices, unique_edges; } kt_mesh_smooth_stats;
int kt_mesh_smooth_create(kt_ctx* ctx, void* hip_stream, kt_mesh_smooth_pass** out);
int kt_mesh_smooth_destroy(kt_mesh_smooth_pass* w);
int kt_mesh_smooth_device(kt_mesh_smooth_pass* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m, int steps,
                          float lambda, float mu, int mode, kt_mesh_vertex* vertices_out_dev, kt_mesh_smooth_stats* stats);
int kt_mesh_smooth(kt_mesh_smooth_pass* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, int steps, float lambda,
                   float mu, int mode, kt_mesh_vertex* vertices_out, kt_mesh_smooth_stats* stats);

/* Renders a mesh from a camera pose: a software rasteriser (kt_mesh_render.hip; restated by kintinuous_amd/mesh_render_ref.py, which the
 * device equals on every byte, on every call).  Input: n vertices, m triangles (uint32[3]), the intrinsics, cols, rows, the camera as
 * kt_tracker_get_pose gives it (R camera-to-world, row-major; t the camera centre) and near (float, metres).
 * Everything below is in double unless stated.  Every product, sum, quotient and conversion is rounded once, in the order written, with
 * nothing contracted; rint rounds ties to even.
 *   - Vertex: d = (double)p - (double)t; c_k = (R[0][k] d.x + R[1][k] d.y) + R[2][k] d.z, which is R^T d (no inverse is taken).  It is
 *     valid under kt_mesh_simplify's rule: x, y, z finite and |coordinate| < 8192.  It is visible when it is valid, c_z >= (double)near
 *     and, with sx = (c_x fx) / c_z + cx and sy = (c_y fy) / c_z + cy, |sx 256| < 2^22 and |sy 256| < 2^22.  Then X = (int32)rint(sx 256),
 *     Y likewise (8 bits of sub-pixel) and iz = 1.0 / c_z.  Pixel (i, j) is sampled at its centre X = 256 i, Y = 256 j: the reference's
 *     rn(x f / z + c) convention.
 *   - Triangle: an index >= n is an error, and so is a referenced vertex that is not valid.  Two equal indices: degenerate, skipped.  A
 *     vertex that is not visible: the whole triangle is skipped and counted as clipped -- there is NO clipping against the near plane or
 *     the guard band.  A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) in int64 (below 2^47): A = 0 is degenerate; with A < 0 vertices 1
 *     and 2 change places (the mesh is drawn two-sided) and everything below uses the order after the swap.  Any other triangle is drawn,
 *     whether or not it covers a pixel.
 *   - Coverage of P = (256 i, 256 j), 0 <= i < cols, 0 <= j < rows: w0 = edge(v1, v2, P), w1 = edge(v2, v0, P), w2 = edge(v0, v1, P),
 *     edge(a, b, P) = (bx - ax)(Py - ay) - (by - ay)(Px - ax) in int64; w0 + w1 + w2 = A.  P is inside when every w_k > 0, or w_k = 0
 *     and the edge a -> b of that w_k is inclusive: by - ay > 0, or by - ay = 0 and bx - ax < 0.  Of a direction and its opposite exactly
 *     one is inclusive, so a centre on the edge two triangles share, or at the vertex of a closed fan, is covered exactly once.
 *   - Depth: S = ((double)w0 iz0 + (double)w1 iz1) + (double)w2 iz2, z = (double)A / S (perspective-correct),
 *     zq = min((int64)rint(z 65536), 2^32 - 2).  The pixel's word is the minimum over all covering triangles of the uint64
 *     zq << 32 | triangle index; all ones means empty.  Equal depth goes to the smaller index; a minimum of integers does not depend on
 *     the scheduling.
 *   - Outputs per pixel, each pointer optional (null: not wanted): index uint32, the winning triangle, 0xFFFFFFFF when empty; depth
 *     uint16 millimetres, min(65535, (zq 1000 + 32768) >> 16), 0 when empty (kt_generate_depth's format; near >= 0.001 keeps a covered
 *     pixel from being 0); color rgb24, per channel rint(((b0 c0 + b1 c1) + b2 c2) / S) clamped to [0, 255] with b_k = (double)w_k iz_k
 *     and c_k the vertex's channel, red the rgb word's bits 16-23 as in kt_host_save_ply; model rgb24 grey, flat per triangle with a
 *     headlight at the camera: nrm = (c1 - c0) x (c2 - c0) of the camera-space vertices, q = (nrm . c0)^2 / ((nrm . nrm)(c0 . c0)), 0
 *     with a zero denominator, g = rint(255 (0.2 + 0.8 q)) -- a squared cosine, so no square root enters the contract; a cross product
 *     is (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), a dot product (x x' + y y') + z z'.  Empty pixels are (0, 0, 0).
 *   - stats: the drawn, clipped and degenerate triangles, the covered pixels.
 * Not covered: clipping (see above), anti-aliasing, smooth shading, points and lines.
 * kt_mesh_render_device: device arrays; everything is enqueued on the object's stream and the host waits once.  kt_mesh_render: the same
 * on host arrays (upload, run, download).
 * KT_ERR_ARG with nothing written to any output or the stats: an index out of range; an invalid referenced vertex (both found on the
 * device); cols or rows outside [1, 8192]; n > 2^29 or m > 2^29; fx, fy, cx, cy, R or t not finite, |t_k| >= 8192, fx or fy not positive;
 * near outside [0.001, 8192); vertices not 16-byte aligned; null inputs with n > 0; an output being or overlapping an input or another
 * output.  n = 0 or m = 0: KT_OK and an empty image.
 * The object owns its workspace (16 bytes per vertex, 8 per pixel, 4 per triangle, the host form's staging), which grows with the calls;
 * hip_stream null: the context's. */
typedef struct kt_mesh_render_pass kt_mesh_render_pass;
typedef struct { uint64_t drawn_triangles, clipped_triangles, degenerate_triangles, covered_pixels; } kt_mesh_render_stats;
int kt_mesh_render_create(kt_ctx* ctx, void* hip_stream, kt_mesh_render_pass** out);
int kt_mesh_render_destroy(kt_mesh_render_pass* w);
int kt_mesh_render_device(kt_mesh_render_pass* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m,
                          const kt_intr* intr, int cols, int rows, const float R[9], const float t[3], float near, uint32_t* index_dev,
                          uint16_t* depth_dev, uint8_t* color_dev, uint8_t* model_dev, kt_mesh_render_stats* stats);
int kt_mesh_render(kt_mesh_render_pass* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, const kt_intr* intr,
                   int cols, int rows, const float R[9], const float t[3], float near, uint32_t* index, uint16_t* depth, uint8_t* color,
                   uint8_t* model, kt_mesh_render_stats* stats);

/* ---- host math of one Gauss-Newton step (no GPU work), for callers that drive kt_icp_step / kt_rgb_step themselves ----
 * dA.ldlt().solve(db)  ICPOdometry.cpp:130 (Eigen LDLT<6x6 double>: pivoted, pseudo-inverse of D); A row-major */
int kt_host_ldlt_solve6(const double A[36], const double b[6], double x[6]);
/* cv::Rodrigues(rvec, R)  OdometryProvider.h:63 */
int kt_host_rodrigues(const double r[3], double R_out[9]);
/* Eigen Matrix3f::inverse()  ICPOdometry.cpp:77 */
int kt_host_mat33_inverse(const float m[9], float out[9]);
/* resultRt = [Rodrigues(x[3..5]) | x[0..2]] * resultRt;  [Rcurr | tcurr] = [Rprev | tprev] * resultRt^-1 (float)
 * ICPOdometry.cpp:133-178 */
int kt_host_pose_update(const double x[6], double resultRt[16], const float Rprev[9], const float tprev[3],
                        float Rcurr[9], float tcurr[3]);
/* K R K^-1 and K t of resultRt^-1 for computeRgbResidual  RGBDOdometry.cpp:213-231 (rigid Mat::inv(DECOMP_SVD), 3x3 products in double) */
int kt_host_compute_krk(const double resultRt[16], double fx, double fy, double cx, double cy, float krkinv[9], float kt[3]);
/* one line of a -p trajectory file {x y z qx qy qz qw} -> Isometry3f {R row-major (9), t (3)}  KintinuousTracker.cpp:244-256 */
void kt_host_trajectory_pose(const float pose7[7], float T[12]);
/* GroundTruthOdometry::getIncrementalTransformation  GroundTruthOdometry.cpp:42-74: A, B = trajectory poses of the previous and the
 * current frame's stamp, (Rlast, tlast) = rmats_.back(), tvecs_.back() */
void kt_host_ground_truth_pose(const float A[12], const float B[12], const float Rlast[9], const float tlast[3], float Rcurr[9],
                               float tcurr[3]);

/* ---- frame-level tracker (KintinuousTracker::processFrame, KintinuousTracker.cpp:444-915) ----
 * Device-resident fast path: the whole per-frame pipeline is enqueued on the context stream, the ICP /
 * RGB-D Gauss-Newton iterations solve and update the pose on the device (no host round trip per
 * iteration).  The host-side C++ class KintinuousTracker (kintinuous_amd/host) is a thin shell over it. */
typedef struct kt_tracker kt_tracker;
typedef struct {
    int cols, rows, N;
    float fx, fy, cx, cy;
    float volume_size;   /* -s  (ConfigArgs.h:117) */
    int voxel_shift;     /* -t  */
    int overlap;         /* 2 = TrackerInterface::enableOverlap(), 0 with -no */
    int static_mode;     /* -sm */
    int use_rgbd;        /* -r  */
    int use_rgbd_icp;    /* -ri */
    int fast_odometry;   /* -fod */
    int disable_color_angle; /* -dc */
    int max_slice_points;    /* 0 = 3 * cols * rows (KintinuousTracker.cpp:77) */
    int dynamic_cube;        /* -d: the cube swings around the camera with its heading (repositionCube, KintinuousTracker.cpp:384-442);
                                the pose is then observed on the host before the frame is fused (no speculative fusion) */
    int place_recognition;   /* a vocabulary file is configured (-v, ConfigArgs::vocabFile): sample frames for the loop-closure
                                backend whenever the camera has moved (rotation + translation) / 2 >= 0.15 since the last sample, or at
                                the next volume shift (KintinuousTracker.cpp:605-624, 706-717), and mark those poses isLoopPose */
} kt_tracker_config;

int kt_tracker_create(kt_ctx* ctx, const kt_tracker_config* cfg, kt_tracker** out);
int kt_tracker_destroy(kt_tracker* t);
int kt_tracker_reset(kt_tracker* t);
/* processFrame with device-resident inputs: depth u16 [rows][cols] (mm), rgb24 [rows][cols][3] */
int kt_tracker_process_frame(kt_tracker* t, const uint16_t* depth_dev, const uint8_t* rgb24_dev, uint64_t timestamp);
/* Optional read-ahead for log playback: announce a frame that a LATER kt_tracker_process_frame call will receive (same two
 * pointers, contents unchanged until then).  Its pose-independent stages (bilateral filter, depth / vertex / normal pyramids,
 * scaleDepth) run on a second HIP stream, overlapped with the fusion of the frame before it.  Up to two announced frames
 * may be outstanding (a third is refused with KT_ERR_STATE); frames may be handed to kt_tracker_process_frame in any order -- an
 * announced frame is found by its pointers, one that is skipped gives its buffers back.  Best issued right before the
 * kt_tracker_process_frame call of the preceding frame.  Results are identical with and without it. */
int kt_tracker_prefetch_frame(kt_tracker* t, const uint16_t* depth_dev, const uint8_t* rgb24_dev);
/* the same for host-resident frames: pinned staging copy + upload + the pose-independent stages, all on the read-ahead stream.  A
 * later kt_tracker_process_frame_host call with the SAME two host pointers consumes it, so outstanding frames need distinct host
 * buffers (the contents are copied here and may change afterwards). */
int kt_tracker_prefetch_frame_host(kt_tracker* t, const uint16_t* depth_host, const uint8_t* rgb24_host);
/* TrackerInterface::process upload path (TrackerInterface.cpp:90-91): host frame -> device -> processFrame */
int kt_tracker_process_frame_host(kt_tracker* t, const uint16_t* depth_host, const uint8_t* rgb24_host, uint64_t timestamp);
/* -p ground-truth odometry.  KintinuousTracker::loadTrajectory (KintinuousTracker.cpp:216-260) without the text parsing:
 * pose7 = n x {x y z qx qy qz qw}, one row per line "utime,x,y,z,qx,qy,qz,qw" of the trajectory file.  From then on the pose of
 * every frame comes from GroundTruthOdometry (GroundTruthOdometry.cpp:42-74) instead of ICP / RGB-D, and a frame whose timestamp
 * has no entry is dropped (preRun, :89-111).  Call before the first frame; repeated calls add entries. */
int kt_tracker_load_trajectory(kt_tracker* t, int n, const uint64_t* utimes_host, const float* pose7_host);
int kt_tracker_finalise(kt_tracker* t);
/* volumeBasis (KintinuousTracker::getVolumeOffset); constant unless dynamic_cube is set */
int kt_tracker_get_volume_basis(kt_tracker* t, float basis_host[3]);
/* KintinuousTracker::repositionCube on explicit state (host code): may move basis[0] and basis[2] */
/* (|rodrigues2(Rcurr^-1 Rlast)| + |cam - camLast|) / 2, KintinuousTracker.cpp:607-611 */
float kt_host_place_recognition_movement(const float Rcurr[9], const float cam[3], const float Rlast[9], const float camLast[3]);
void kt_host_reposition_cube(const float R[9], const float tlast[3], float volume_size, const float voxel_size[3], int thresh, float basis[3]);
/* rmats_.back() (row-major 3x3), tvecs_.back(), currentGlobalCamera */
int kt_tracker_get_pose(kt_tracker* t, float R_host[9], float t_host[3], float global_cam_host[3]);
int kt_tracker_num_poses(kt_tracker* t);   /* (the kt_tracker_num_* counts are -1 when the frame in flight failed: kt_last_error()) */
/* densePoseGraph[i]: timestamp, row-major 4x4 [R | currentGlobalCamera], isLoopPose */
int kt_tracker_get_dense_pose(kt_tracker* t, int i, uint64_t* ts, float pose16_host[16], int* is_loop);
int kt_tracker_get_voxel_wrap(kt_tracker* t, int wrap_host[3]);
int kt_tracker_num_slices(kt_tracker* t);
int kt_tracker_slice_info(kt_tracker* t, int i, size_t* n_points, int* dimension);
int kt_tracker_slice_points(kt_tracker* t, int i, kt_point_xyzrgb* out_host);
/* the CloudSlice's cameraRotation (row-major), cameraTranslation (= currentGlobalCamera) and utime, CloudSlice.h:110-115 */
int kt_tracker_slice_pose(kt_tracker* t, int i, float R_host[9], float cam_host[3], uint64_t* ts);
/* setParked (KintinuousTracker.cpp:988-991): a parked tracker never shifts */
int kt_tracker_set_parked(kt_tracker* t, int parked);
/* device pointers of the tracker's volume / maps, for inspection and parity tests */
int16_t* kt_tracker_volume(kt_tracker* t);
uint8_t* kt_tracker_color_volume(kt_tracker* t);
float* kt_tracker_vmap_g_prev(kt_tracker* t, int level);
float* kt_tracker_nmap_g_prev(kt_tracker* t, int level);
/* vmap_curr_color: the raycast's uchar4 colour + weight image of the last frame (input of kt_generate_image) */
uint8_t* kt_tracker_vmap_curr_color(kt_tracker* t);
float kt_tracker_trunc_dist(kt_tracker* t);
/* profiling: on = 0 off, 2 = all stages, 1 / 5 / 6 / 4 = only the tsdf23 voxel kernel, on every 8th / 4th / 2nd / every frame (an event
 * pair is two marker packets on the main stream, ~10 us of bubbles: timing every frame lowers the frame rate it is measured next to).
 * kt_tracker_stage_ms returns the MEAN milliseconds per frame since profiling was enabled (hipEvent pairs on
 * the context stream) for: 0 pyramid, 1 odometry, 2 shift, 3 integrate (scaleDepth + tsdf23), 4 raycast,
 * 5 predicted-map resize, 6 the tsdf23 kernel alone; kt_tracker_stage_counts the number of samples of each. */
int kt_tracker_enable_profiling(kt_tracker* t, int on);
int kt_tracker_stage_ms(kt_tracker* t, float ms_host[7]);
int kt_tracker_stage_counts(kt_tracker* t, long long n_host[7]);
/* where the host thread spends a frame: mean seconds per kt_tracker_process_frame call {whole call, waiting for the previous
 * frame's pose}; reset != 0 restarts the statistics */
int kt_tracker_host_times(kt_tracker* t, double out2_host[2], int reset);
/* counters of the last frame (costs two extra syncs per frame; off by default): U = voxels that passed the
 * integrate update predicate, S = ray-march steps */
int kt_tracker_enable_counts(kt_tracker* t, int on);
int kt_tracker_last_counts(kt_tracker* t, unsigned long long* U, unsigned long long* S);
/* Frames whose voxel pass ran from a task plan made ahead of the frame for a predicted pose {hits}, and frames whose pose fell outside
 * the plan's margins and were fused through the in-stream pre-pass instead {misses} (csrc/kt_volume.hip "planning ahead"; results do
 * not depend on which of the two happened). */
int kt_tracker_plan_stats(kt_tracker* t, long long out2_host[2]);
/* Frames whose odometry was run a second time, one launch per iteration, because an inter-workgroup hand-off of the first attempt gave up
 * (csrc/kt_track.hip: kt_icp_level_kernel needs its whole grid resident; another process on the same GPU can keep a workgroup out).  The
 * reference's icpStep is stream-ordered and cannot fail this way (reduce.cu:347-419); here the frame is re-run inside the call that observes
 * it, with the same bits, and only counted.  0 on an undisturbed GPU. */
int kt_tracker_odometry_fallbacks(kt_tracker* t, long long* out_host);


/* The per-slice stage of the backend's CloudSliceProcessor (backend/CloudSliceProcessor.cpp:87-163), the consumer right behind every
 * volume shift: keep points with alpha >= weight_cull (if weight_cull > 0; ConfigArgs::weightCull), pcl::VoxelGrid down-sampling at
 * `leaf` (the voxel size, :124-130), pcl::NormalEstimation with the k (= 20, :148) nearest neighbours, normals flipped towards the sensor
 * origin, output pcl::PointXYZRGBNormal in leaf order.  points_host / out_host are host arrays (a CloudSlice's cloud / processedCloud);
 * out_host needs room for n points; *n_out receives the count. */
int kt_slice_process(kt_ctx* ctx, const kt_point_xyzrgb* points_host, size_t n, int weight_cull, float leaf, int k,
                     kt_point_xyzrgbnormal* out_host, size_t* n_out);
/* The same stage on device-resident points ("slab points are already on device"), asynchronous on the workspace's own
 * stream (or `hip_stream`), with every intermediate -- the input count, the leaf grid, the output count -- kept on the device:
 *   kt_slice_ws_create      buffers for up to `capacity` input points, allocated once;
 *   kt_slice_process_device points_dev[0 .. *n_dev), n_dev a DEVICE word (e.g. the extraction kernel's counter), n_max a host-known
 *                           upper bound of it; enqueues the stage and returns;
 *   kt_slice_ws_count       waits for the stream; *n_out = number of output points, which are kt_slice_ws_output(ws)[0 .. *n_out)
 *                           (device memory, valid until the next call on the workspace).
 * kt_tracker_enable_slice_stage puts it behind the tracker's own shift path. */
typedef struct kt_slice_ws kt_slice_ws;
int kt_slice_ws_create(kt_ctx* ctx, size_t capacity, void* hip_stream, kt_slice_ws** out);
int kt_slice_ws_destroy(kt_slice_ws* ws);
void* kt_slice_ws_stream(kt_slice_ws* ws);
int kt_slice_process_device(kt_slice_ws* ws, const kt_point_xyzrgb* points_dev, const unsigned int* n_dev, size_t n_max, int weight_cull, float leaf, int k);
int kt_slice_ws_count(kt_slice_ws* ws, size_t* n_out);
const kt_point_xyzrgbnormal* kt_slice_ws_output(kt_slice_ws* ws);

/* CloudSliceProcessor::save (backend/CloudSliceProcessor.cpp:180-231), host code, once per run:
 * kt_host_voxel_grid_normal = the pcl::VoxelGrid<pcl::PointXYZRGBNormal> at `leaf` it applies to the concatenated processed clouds when
 * extractOverlap && !saveOverlap (:197-218; every field averaged per leaf, rgb re-packed with a zero alpha byte, leaves in key order);
 * out needs room for n points.  kt_host_save_pcd = pcl::io::savePCDFile(path, cloud, true) (:224-226): PCD v0.7, DATA binary,
 * FIELDS x y z rgb normal_x normal_y normal_z curvature, 32 bytes per point. */
int kt_host_voxel_grid_normal(const kt_point_xyzrgbnormal* in, size_t n, float leaf, kt_point_xyzrgbnormal* out, size_t* n_out);
int kt_host_save_pcd(const char* path, const kt_point_xyzrgbnormal* points, size_t n);
/* a mesh as binary little-endian PLY 1.0: element vertex {float x, y, z; uchar red, green, blue} (red = rgb bits 16-23, kt_point_xyzrgb's
 * r byte; blue = bits 0-7), element face {list uchar int vertex_indices}.  Several slices' meshes are saved as one by concatenating
 * them in slice order with the triangle indices offset by the vertices before them (the shape of MeshGenerator.cpp:82-137's merge). */
int kt_host_save_ply(const char* path, const kt_mesh_vertex* vertices, size_t n_vertices, const uint32_t* triangles, size_t n_triangles);
/* the same mesh with the normals of kt_mesh_normals: element vertex {float x, y, z, nx, ny, nz; uchar red, green, blue}, 27 bytes per
 * vertex; the face element and the index check are kt_host_save_ply's */
int kt_host_save_ply_normals(const char* path, const kt_mesh_vertex* vertices, const kt_mesh_normal* normals, size_t n_vertices,
                             const uint32_t* triangles, size_t n_triangles);

/* The slice stage behind the tracker's own shift path: from this call on every extracted slab also goes through
 * kt_slice_process_device(weight_cull, leaf = the largest voxel edge, k) on a stream of its own (the slab never leaves the device in
 * between), and its CloudSlice::processedCloud travels with the slice.  kt_tracker_slice_processed_info: the number of processed points
 * of slice i, -1 for a slice extracted while the stage was off. */
int kt_tracker_enable_slice_stage(kt_tracker* t, int on, int weight_cull, int k);
int kt_tracker_slice_processed_info(kt_tracker* t, int i, long long* n_points);
int kt_tracker_slice_processed(kt_tracker* t, int i, kt_point_xyzrgbnormal* out);

/* The mesh stage behind the shift path (the -m switch; marching cubes, not the reference's greedy projection): from this call on
 * every fetched slab is also meshed with kt_extract_mesh's rules, on the context stream right after its extraction and before the
 * clears, with the slice's own real_voxel_wrap; the download rides the slice's helper-thread job.  The box along the shifted axis is
 * every cell with a corner in the voxel range that LEAVES the volume: [0, vt) for a plus shift, [N + vt - 1, N - 1) for a minus one
 * (all cells [0, N - 1) across); kt_tracker_finalise meshes [0, N - 1)^3.  So no cell is meshed twice.  The clears reset one plane
 * more than leaves (kt_clear_volume); that plane stays as the new logical 0 / |vt| and is meshed later once fused again -- where it
 * is not, a one-cell gap remains.  Both slabs emit a vertex on the in-plane edges of that plane: the slices' meshes are separate, and
 * kt_mesh_weld joins them by the keys of kt_tracker_enable_mesh_keys.  max_vertices / max_triangles
 * bound each slice's mesh (0 = 8 * N * N vertices and twice as many triangles); turning the stage off frees nothing until it is
 * turned on again with other bounds.
 * kt_tracker_slice_mesh_info: the true sizes of slice i's mesh, -1 for a slice taken with the stage off;
 * kt_tracker_slice_mesh copies it (vertices, triangles: host arrays of those sizes), KT_ERR_CAPACITY when it exceeded the bounds.
 * kt_tracker_enable_mesh_keys: from this call on the stage also keeps each slab's edge keys (kt_extract_mesh_keyed's, under the slice's
 * real_voxel_wrap) beside its vertices: one more pinned array per download buffer, filled by the same kernel and moved by the same
 * helper-thread job.  Off (the default) the stage does exactly what it does without this call.  KT_ERR_ARG from the frame that shifts
 * once a global voxel leaves [-2^19, 2^19).
 * kt_tracker_slice_mesh_keys copies slice i's keys (a host array of n_vertices entries): KT_ERR_STATE for a slice meshed without keys,
 * KT_ERR_CAPACITY where kt_tracker_slice_mesh returns it. */
int kt_tracker_enable_mesh_stage(kt_tracker* t, int on, long long max_vertices, long long max_triangles);
int kt_tracker_slice_mesh_info(kt_tracker* t, int i, long long* n_vertices, long long* n_triangles);
int kt_tracker_slice_mesh(kt_tracker* t, int i, kt_mesh_vertex* vertices, uint32_t* triangles);
int kt_tracker_enable_mesh_keys(kt_tracker* t, int on);
int kt_tracker_slice_mesh_keys(kt_tracker* t, int i, uint64_t* keys);

/* Place-recognition tap (KintinuousTracker::addToPlaceRecognition, KintinuousTracker.cpp:917-958): the frames sampled for the
 * loop-closure backend, in order.  The library keeps the sample's metadata (PlaceRecognitionInput::utime / trans / rotation and the
 * index of the dense pose it belongs to); the caller, who owns the frame buffers, copies the image and depth of that frame
 * (host/KintinuousTracker.h fills placeRecognitionBuffer from them).  slice_pr_id: the sample attached to slice i as its
 * placeRecognitionFrame (mutexOutCloudBuffer's last argument, finalise :1038-1045), or -1. */
int kt_tracker_num_pr_samples(kt_tracker* t);
int kt_tracker_pr_sample(kt_tracker* t, int i, uint64_t* utime, float trans[3], float rotation[9], int* pose_index);
int kt_tracker_slice_pr_id(kt_tracker* t, int i, int* pr_id);

/* ---- the dense registration of a loop-closure candidate (kt_loop.hip) ----
 * kt_loop_icp_depth_frames replaces PlaceRecognition::icpDepthFrames (backend/PlaceRecognition.cpp:238-276, the "LoopConstraint" stage):
 * frame1 (the old image) and frame2 (the new one) are host arrays of rows x cols uint16 millimetres.
 *   a. cloud (DepthCamera::convertToXYZPointCloud, backend/DepthCamera.cpp:143-163): a pixel is kept when d != 0 && d < max_dist * 1000
 *      (the reference's default max_dist is 4.0); z = d * 0.001f, x = ((float)u - cx) * z * (1.0f / fx), y likewise, in float with
 *      the kt_intr floats (the reference mixes double intrinsics into that product); points in the reference's order, column outer.
 *   b. pcl::VoxelGrid<PointXYZ> at `leaf` (the caller passes 2.5 x the voxel edge, :250) with kt_slice_process's rules: the points of a
 *      leaf summed in input order, leaves in key order.  This gives the clouds S (frame1) and T (frame2).
 *   c. M = bootstrap (row-major 4x4), kept in double.  Every pass moves S by M (double product, rounded to float once per coordinate),
 *      finds for every point its exact nearest neighbour in T under d^2 = (dx * dx + dy * dy) + dz * dz in float -- ties to the lowest
 *      index, no distance cap -- reduces the 15 sums of the point-to-point problem in double in a fixed order, and the host solves the
 *      closed-form rigid fit (kt_host_rigid_fit) and sets M = dM M.  It stops after max_iterations updates (PCL's default is 10), or at
 *      the first pass whose correspondences equal the previous pass's: a fixed point, that pass updates nothing (converged = 1).
 *   d. score = the mean of d^2 to the nearest neighbour under the final M (pcl getFitnessScore with its default range), summed in double.
 * DIVERGENCE FROM PCL: pcl::IterativeClosestPointNonLinear minimises the same point-to-point error by Levenberg-Marquardt and stops on
 * its own epsilons; this stage takes the closed-form optimum of every step and stops at the fixed point.  Same objective, not the same
 * iterates: results agree with PCL's only as far as both have converged.
 * out_transform = the reference's icp.getFinalTransformation() * bootstrap.  If either cloud is empty: KT_OK, out_transform = bootstrap,
 * score = +inf, iterations = 0 (a caller comparing against the reference's 0.01 gate rejects the constraint).  Synchronises. */
typedef struct { int n_source, n_target, iterations, converged; } kt_loop_icp_info;
int kt_loop_icp_depth_frames(kt_ctx* ctx, const uint16_t* frame1, const uint16_t* frame2, int cols, int rows, const kt_intr* intr,
                             const float bootstrap[16], float leaf, float max_dist, int max_iterations, float out_transform[16],
                             float* out_score, kt_loop_icp_info* out_info);
/* steps a + b for one frame (DepthCamera.cpp:143-163 + PlaceRecognition.cpp:248-256): out_xyz = a host array of `capacity` points of 3
 * floats; *n_out = the true number of points.  If it exceeds capacity NOTHING is written and KT_ERR_CAPACITY is returned.  Same
 * divergences as above: float intrinsics, PCL's unspecified in-leaf summation order fixed to input order. */
int kt_depth_to_cloud_grid(kt_ctx* ctx, const uint16_t* frame, int cols, int rows, const kt_intr* intr, float leaf, float max_dist,
                           float* out_xyz, size_t capacity, size_t* n_out);
/* the correspondence search of step c alone (PCL: CorrespondenceEstimation over a kd-tree, PlaceRecognition.cpp:264-266; here an exact
 * brute-force search with a defined tie rule): host clouds of n_src / n_dst points (both > 0) of 3 floats, out_index[i] = the lowest
 * index of a nearest point of dst to src[i], out_d2[i] = its squared distance; host arrays of n_src entries. */
int kt_cloud_nearest(kt_ctx* ctx, const float* src_xyz, size_t n_src, const float* dst_xyz, size_t n_dst, uint32_t* out_index, float* out_d2);
/* the host half of step c (no GPU work): the rigid dM (row-major 4x4, det R = +1) minimising sum |dM s_i - t_i|^2 over n pairs from
 * sums = {sum s (3), sum t (3), sum s t^T (9: source row, target column)}, by Horn's unit quaternion with a Jacobi eigen-solver in
 * double.  PCL reaches the same optimum iteratively (TransformationEstimationLM). */
int kt_host_rigid_fit(const double sums[15], double n, double dM[16]);

/* ---- the bootstrap of a loop-closure candidate: features, matches, RANSAC (kt_match.hip) ----
 * kt_loop_match_frames takes the place of the dense half of PlaceRecognition::processLoopClosureDetection before icpDepthFrames
 * (backend/PlaceRecognition.cpp:114-188): SURF keypoints and descriptors (DBowInterfaceSurf), their 3D points and ratio-test match
 * (Surf3DTools.h:67-270) and cv::solvePnPRansac at 500 iterations / 2 px (PNPSolver.cpp:32-97).  It is a DEFINED STAGE with the
 * reference's inputs, outputs and gates, NOT a port of SURF or of OpenCV's PnP: every step is integer arithmetic or uncontracted float /
 * double arithmetic of a fixed order, so kintinuous_amd/loop_match_ref.py restates it bit for bit.  Frames are host arrays: rgb24
 * rows x cols x 3 bytes, depth rows x cols uint16 millimetres.
 *   a. intensity: kt_bgr_to_intensity's rule on the rgb24 image (the reference: cv::cvtColor RGB2GRAY, other weights and rounding).
 *   b. keypoints: FAST-9 on the 16-pixel Bresenham ring of radius 3 -- p is a corner when 9 contiguous ring pixels are all > I_p + t or
 *      all < I_p - t (t = fast_threshold); score = sum over the ring of max(|I_r - I_p| - t, 0).  Non-maximum suppression over the 8
 *      neighbours on the scores of ALL corners: strictly greater than the neighbours earlier in raster order, greater or equal to the
 *      later ones.  A surviving corner is kept when it lies at least 15 pixels (13 of descriptor reach + 2 of the box) from every border
 *      and its depth d satisfies d != 0 && d < max_dist * 1000 (step a of the registration stage; Surf3DTools.h:86 drops keypoints
 *      without depth).  The max_keypoints (<= 4096) best by (score descending, raster index ascending) are output, in that order.
 *   c. descriptors: upright BRIEF-256 on S = the 5x5 box SUM of the intensity (uint16, no division): bit k = S(p + a_k) < S(p + b_k) for
 *      the 256 offset pairs of csrc/kt_brief_table.hpp (kintinuous_amd/brief_table.py generates it: splitmix64, fixed seed), eight
 *      uint32 words per keypoint, bit k in word k / 32 at position k % 32.
 *   d. 3D points: z = d * 0.001f, x = ((float)u - cx) * z * (1.0f / fx), y likewise (step a of the registration stage).
 *   e. matching (surfMatch3D's role): for every NEW keypoint the nearest and second-nearest OLD descriptor by Hamming distance, ties to
 *      the lowest index; d1, d2 = the two smallest distances, duplicates counted (with ONE old descriptor there is no second neighbour:
 *      d2 = 257, one more than any distance of 256 bits).  Accepted when d1 <= max_hamming && ratio_den * d1 < ratio_num * d2 (the integer
 *      ratio stands in for the reference's 0.49 on squared L2) and the old keypoint's nearest new keypoint is this one (cross-check, same
 *      tie rule).  Matches are listed in new-keypoint order.
 *   f. RANSAC (PNPSolver::getRelativePose's role): n_hypotheses hypotheses (the reference's 500).  Hypothesis h draws three distinct
 *      match indices from r_k = fmix32(seed + 0x9E3779B9 * (3 h + k + 1)) (murmur3's finaliser, mod 2^32): i0 = r_0 % M,
 *      i1 = r_1 % (M - 1) skipping i0, i2 = r_2 % (M - 2) skipping both.  The rigid T (new-camera 3D -> old-camera 3D) through the three
 *      pairs comes from orthonormal triads in double: e1 = (p1 - p0) / |.|, e3 = e1 x (p2 - p0) / |.|, e2 = e3 x e1 on both sides,
 *      R = F_old F_new^T, t = c_old - R c_new with c the triple's centroid; a triple with a norm below 1e-3 scores 0.  Score = the matches
 *      whose new 3D point, moved by T and projected with the intrinsics (u = (fx X) / Z + cx in double), has Z > 0 and lies within
 *      reproj_px of the old keypoint (squared error <= reproj_px^2; the reference's 2.0).  Best = the highest score, ties to the lowest
 *      hypothesis.  The host refits over the best hypothesis's inliers with kt_host_rigid_fit (sums in double, in match order) and
 *      scores once more: that gives the final T and the final inlier flags.
 * out_pose = T as float (row-major 4x4); out_bootstrap = float(the rigid inverse of T, in double): the reference's
 * T.cast<float>().inverse(), old -> new, which is what kt_loop_icp_depth_frames takes.  out_matches: match_capacity x 4 ints (old u, old
 * v, new u, new v); out_inlier: match_capacity bytes.  More matches than match_capacity (max_keypoints always suffices): out_info holds
 * the counts, nothing else is written, KT_ERR_CAPACITY.  Fewer than 3 matches, or no hypothesis scoring at least 3: KT_OK, pose and
 * bootstrap = identity, n_inliers = 0, best_hypothesis = -1.  The gates (40 matches, the inlier share) are the caller's, as in the
 * reference.  Synchronises. */
typedef struct {
    int fast_threshold, max_keypoints, max_hamming, ratio_num, ratio_den, n_hypotheses;
    float reproj_px, max_dist;
    uint32_t seed;
} kt_loop_match_params;
typedef struct { int n_kp_old, n_kp_new, n_matches, n_inliers, best_hypothesis; } kt_loop_match_info;
/* fast_threshold 20, max_keypoints 2048, max_hamming 64, ratio 4 / 5, n_hypotheses 500, reproj_px 2.0, max_dist 4.0, seed 1 */
int kt_loop_match_params_default(kt_loop_match_params* params);
int kt_loop_match_frames(kt_ctx* ctx, const uint8_t* rgb_old, const uint16_t* depth_old, const uint8_t* rgb_new, const uint16_t* depth_new,
                         int cols, int rows, const kt_intr* intr, const kt_loop_match_params* params, float out_pose[16],
                         float out_bootstrap[16], int32_t* out_matches, uint8_t* out_inlier, size_t match_capacity,
                         kt_loop_match_info* out_info);
/* steps a - c for one frame: out_uv = capacity x 2 ints (u, v), out_score = capacity ints, out_desc = capacity x 8 uint32; *n_out = the
 * true number of keypoints.  If it exceeds capacity NOTHING is written and KT_ERR_CAPACITY is returned. */
int kt_frame_keypoints(kt_ctx* ctx, const uint8_t* rgb24_host, const uint16_t* depth_host, int cols, int rows,
                       const kt_loop_match_params* params, int32_t* out_uv, int32_t* out_score, uint32_t* out_desc, size_t capacity,
                       size_t* n_out);
/* step e without the cross-check, on host arrays of n_new / n_old (both > 0) descriptors of 8 uint32: out_old_index[i] = the old index
 * accepted for new descriptor i or -1, out_d1 / out_d2 its two smallest distances (d2 = 257 when n_old == 1); arrays of n_new ints. */
int kt_descriptor_match(kt_ctx* ctx, const uint32_t* desc_new, size_t n_new, const uint32_t* desc_old, size_t n_old,
                        const kt_loop_match_params* params, int32_t* out_old_index, int32_t* out_d1, int32_t* out_d2);

/* ---- the source of loop-closure candidates: a descriptor database (kt_loopdb.hip) ----
 * kt_loop_db takes the place of PlaceRecognition::process's dbowInterface->detectLoop() (backend/PlaceRecognition.cpp:51-88), which
 * DBowInterfaceSurf.cpp:34-45 configures as a DLoopDetector over SURF words (use_nss, alpha = 0.3, k = 1, room for 1000 entries).  It is a
 * DEFINED STAGE with that detector's role, inputs and outputs, NOT a port of DBoW2 / DLoopDetector: no vocabulary, no inverted index.
 * All arithmetic is integer; kintinuous_amd/loop_db_ref.py restates it bit for bit.
 *   database   max_entries entries, numbered from 0 in insertion order; an entry is the descriptor list of one frame as kt_frame_keypoints
 *              outputs it (n <= max_keypoints descriptors of 8 uint32).  One device arena of max_entries * max_keypoints * 32 bytes and a
 *              count per entry, allocated at creation.  It never grows: an insertion into a full database returns KT_ERR_CAPACITY and
 *              changes nothing.
 *   score      s(q, e) = the number of query descriptors accepted against entry e under kt_descriptor_match's rule: d1, d2 the two
 *              smallest Hamming distances to e's descriptors (duplicates counted, d2 = 257 when e holds one), accepted when
 *              d1 <= max_hamming && ratio_den * d1 < ratio_num * d2.  No cross-check.  An empty entry or an empty query scores 0.
 *   detection  for a query with newest = size - 1 (before the query is appended):
 *              1. size == 0: EMPTY.
 *              2. r = s(q, newest), the normaliser (use_nss's similarity to the previous image); r < min_score: LOW_REFERENCE.
 *              3. e is a candidate when e <= newest - dislocal && s(q, e) >= min_score && alpha_den * s(q, e) >= alpha_num * r; none:
 *                 NO_CANDIDATE.
 *              4. islands = maximal runs of candidates whose consecutive ids differ by at most max_gap; an island's score = the sum of
 *                 its members' s.  Best island: the highest sum, ties to the lowest first id; best entry: the highest s in it, ties to
 *                 the lowest id.
 *              5. consistency = 1: DETECTED only if the immediately preceding detect call on this database reached step 4 too and
 *                 [first - max_gap, last + max_gap] of its best island and of this one share an id; otherwise NOT_CONSISTENT.  The island
 *                 is remembered either way (a call that stops before step 4 forgets it).  consistency = 0 skips this step.
 *              6. the query is appended as entry `size`.
 * alpha_num / alpha_den, consistency and the 1000 entries are the reference's; min_score is the caller's 40-match gate; dislocal and max_gap
 * are this project's choices.  The geometric check of a candidate is the caller's (LoopClosureDetection.h). */
#define KT_LOOP_DB_EMPTY 0
#define KT_LOOP_DB_LOW_REFERENCE 1
#define KT_LOOP_DB_NO_CANDIDATE 2
#define KT_LOOP_DB_NOT_CONSISTENT 3
#define KT_LOOP_DB_DETECTED 4
typedef struct { int dislocal, alpha_num, alpha_den, min_score, max_gap, consistency; } kt_loop_db_detect_params;
/* entry = the id the query got; candidate = the best entry when status is DETECTED, else -1; candidate_score = the best entry's s and
 * island_* = the best island when step 4 was reached, else 0 and -1, -1, 0; reference_score = r (0 when EMPTY); n_keypoints = the query's
 * descriptor count (kt_host_loop_db_select leaves it 0). */
typedef struct { int entry, status, candidate, candidate_score, reference_score, island_first, island_last, island_score, n_keypoints; } kt_loop_db_result;
typedef struct kt_loop_db kt_loop_db;
/* dislocal 20, alpha 3 / 10, min_score 40, max_gap 3, consistency 1 */
int kt_loop_db_detect_params_default(kt_loop_db_detect_params* params);
/* bound to hip_stream (null: the context's stream): every copy and launch of the database goes there, and every call below waits for it
 * before returning.  1 <= max_entries <= 2^20.  match_params: max_keypoints sizes an entry, the rule is the score's. */
int kt_loop_db_create(kt_ctx* ctx, int max_entries, const kt_loop_match_params* match_params, void* hip_stream, kt_loop_db** out);
int kt_loop_db_destroy(kt_loop_db* db);
int kt_loop_db_reset(kt_loop_db* db);   /* size 0, the remembered island forgotten: as new */
int kt_loop_db_size(kt_loop_db* db);    /* -1 for a null database */
/* extracts the frame's keypoints (kt_frame_keypoints' steps a - c, on the context's workspace and stream; the database's stream waits for
 * them on the device), scores them against every entry in ONE launch, selects on the host and appends.  A full database:
 * KT_ERR_CAPACITY before any work. */
int kt_loop_db_detect(kt_loop_db* db, const uint8_t* rgb24_host, const uint16_t* depth_host, int cols, int rows,
                      const kt_loop_db_detect_params* detect_params, kt_loop_db_result* out_result);
/* appends n (0 <= n <= max_keypoints) host descriptors as a new entry, *out_entry = its id; detection state is not touched */
int kt_loop_db_add_descriptors(kt_loop_db* db, const uint32_t* desc_host, size_t n, int* out_entry);
/* s(q, e) for e = first .. last (0 <= first <= last < size) of n host descriptors into out_scores_host[0 .. last - first]: no selection,
 * no append.  A bad range or n > max_keypoints: KT_ERR_ARG, nothing launched. */
int kt_loop_db_scores(kt_loop_db* db, const uint32_t* desc_host, size_t n, int first, int last, int32_t* out_scores_host);
/* reads entry e back: *n_out = its count; more than capacity: NOTHING is written, KT_ERR_CAPACITY */
int kt_loop_db_entry(kt_loop_db* db, int e, uint32_t* out_desc_host, size_t capacity, size_t* n_out);
/* steps 1 - 5 alone, no GPU work: scores[0 .. size) = s(q, e); prev_island = {first, last} of the preceding call's best island, or null /
 * first < 0 for none.  out_result->entry = size. */
int kt_host_loop_db_select(const int32_t* scores, int size, const int32_t prev_island[2], const kt_loop_db_detect_params* detect_params,
                           kt_loop_db_result* out_result);

/* ---- the consumer of the accepted loop constraints: the dense pose graph (kt_posegraph.hip) ----
 * kt_pose_graph takes the place of iSAMInterface's graph and its batch_optimization() (backend/iSAMInterface.cpp, driven by
 * Deformation::addCameraCamera / addCameraLoop, backend/Deformation.cpp:130-346).  It is a DEFINED STAGE with the reference's role, inputs,
 * outputs and acceptance rule, NOT a port of iSAM: no Euler-angle Pose3d, no transformation2isam basis change, no QR.
 * kintinuous_amd/pose_graph_ref.py restates it in the same operation order.
 *   graph      nodes 0 .. n_nodes - 1 with poses T_k (camera to world, row-major 4x4 doubles); node 0 is fixed at T0 (the reference's prior
 *              factor); chain_Z[k - 1] (k = 1 .. n_nodes - 1) measures T_{k-1}^-1 T_k; loop l measures T_a^-1 T_b with a != b in either
 *              order (a swapped pair is normalised to a < b with the rigid inverse of its measurement).  For a LoopClosureConstraint a is
 *              the node of time1 (the new frame), b the node of time2, Z = icpTrans (Pose3d_Pose3d_Factor(node1, node2, delta)).
 *   cost       for an edge (i, j, Z): E = Z^-1 T_i^-1 T_j, r = [trans(E); Log_SO3(rot(E))], C = sum |r|^2 over all edges, chi2 = 1000 C
 *              (every factor of the reference has covariance 1e-3 I).  Log_SO3 is taken away from pi: the residuals of a graph worth
 *              optimising are small.
 *   start      T_k = T0 Z_1 ... Z_k: a call does not depend on the one before it (batch_optimization).
 *   solver     Gauss-Newton over the increments D_k = T_{k-1}^-1 T_k, D_k <- D_k Exp(delta_k) with Exp([v; w]) = [Exp_SO3(w) | v]; the
 *              chain's normal matrix is block diagonal and the loops enter through the 6L x 6L matrix S = I + A H^-1 A^T.
 *              It stops when max |delta|_inf < 1e-9 (KT_POSE_GRAPH_CONVERGED) or after 20 steps (KT_POSE_GRAPH_MAX_STEPS).  All steps are
 *              enqueued at once and the host waits once.  Doubles in a fixed order, no floating-point atomics: the same input gives the
 *              same bytes on every call.
 *              The solver works in the frame of node 0 (T0 is applied to the result), so accuracy does not depend on where the world's origin
 *              is, only on the extent d of the trajectory: about d^2 x 1e-16 of S's entries is lost to the adjoints' lever arms.
 * n_loops = 0 (and so n_nodes = 1) is valid: poses_out = the start, steps = 0, converged.  More nodes or loops than the object was created
 * for: KT_ERR_CAPACITY before any work, nothing written.  max_loops <= 64. */
typedef enum { KT_POSE_GRAPH_CONVERGED = 0, KT_POSE_GRAPH_MAX_STEPS = 1 } kt_pose_graph_status;
typedef struct { double chi2_start, chi2_end; int steps, status; } kt_pose_graph_result;
typedef struct kt_pose_graph kt_pose_graph;
/* bound to hip_stream (null: the context's stream): every copy and launch goes there */
int kt_pose_graph_create(kt_ctx* ctx, int max_nodes, int max_loops, void* hip_stream, kt_pose_graph** out);
int kt_pose_graph_destroy(kt_pose_graph* pg);
/* host arrays: T0 16 doubles, chain_Z (n_nodes - 1) x 16, loop_a / loop_b n_loops ints, loop_Z n_loops x 16, poses_out n_nodes x 16 */
int kt_pose_graph_optimise(kt_pose_graph* pg, int n_nodes, const double T0[16], const double* chain_Z, int n_loops, const int* loop_a,
                           const int* loop_b, const double* loop_Z, double* poses_out, kt_pose_graph_result* result);
/* a chain or loop measurement from two float poses (row-major 4x4), no GPU work: Z = prev^-1 curr in double, each rotation block first
 * replaced by the rotation of its normalised quaternion (float matrices are not exactly orthonormal; the quaternion is taken from the
 * largest of {trace, R00, R11, R22}), the inverse being the rigid [R^T | -R^T t] */
int kt_host_pose_graph_measurement(const float prev16[16], const float curr16[16], double Z16[16]);

/* ---- the consumer of the optimised trajectory: the deformation graph of the map (kt_deform.hip) ----
 * kt_deform takes the place of DeformationGraph (backend/DeformationGraph.cpp: initialiseGraphPoses, optimiseGraphSparse,
 * applyGraphToVertices, driven by Deformation::addCameraLoop, backend/Deformation.cpp:258-334).  A DEFINED STAGE with the reference's
 * energy, graph, weights and constants, NOT a port: no CHOLMOD, no PCL, no incremental bookkeeping.  kintinuous_amd/deform_ref.py restates
 * it in the same operation order.
 *   graph      n_nodes >= 5 nodes in time order: positions (3 floats each, widened to double) and strictly increasing times.  The state is 12
 *              doubles per node in the reference's column order: A column-major (entry 3 c + r = A(r, c)), then b; identity = A = I, b = 0.
 *              Neighbours (connectGraphSeq, k = 4): i - 1, i + 1, i - 2, i + 2; the first two nodes take {0..4} \ {i}, the last two the last five.
 *   weights    of a vertex (p, t), map points and constraint sources alike (weightVerticesSeq): `found` = the node nearest in time (|dt| on
 *              signed 64-bit values, a tie to the lower index); the window found, found - 1, ... (at most 20 nodes), topped up with found + 1,
 *              ... to 20 while nodes last; float distances sqrtf((dx dx + dy dy) + dz dz) ordered by (distance, index); dMax = the fifth
 *              smallest; the four nearest get w = (1 - d / dMax)^2 with d the double norm to the node's double position, divided by their
 *              sum in order of nearness; all four 0.25 when that sum is 0 or not finite.  Stored as int32[4] node indices ascending and
 *              double[4] weights.  + - * / and sqrt alone: the restatement agrees bit for bit.
 *   energy     sparseResidual / sparseJacobian with wRot = 1, wReg = 10, wCon = 100: six E_rot rows per node, three E_reg rows per (node,
 *              neighbour), sqrt(wReg) (A_j (g_n - g_j) + g_j + b_j - g_n - b_n), three E_con rows per constraint,
 *              sqrt(wCon) (sum w_i (A_i (s - g_i) + g_i + b_i) - target).  error = the squared norm of all rows.
 *   steps      optimiseGraphSparse, from the identity state: constraint_error = |r_con| / n_con; below params->significant_error nothing is
 *              deformed (KT_DEFORM_INSIGNIFICANT, the state stays identity).  Otherwise at most max_steps Gauss-Newton steps (the normal
 *              equations in band storage, a direct banded L D L^T on the device), stopping after a step when |delta| < delta_tol, error <
 *              error_tol or |error - lastError| < change_tol error (KT_DEFORM_CONVERGED), else KT_DEFORM_MAX_STEPS.  All steps are enqueued at
 *              once and the host waits once.  The trajectory must bend and three constraints must lie out of line: on a straight line of
 *              nodes the rotation about the line is free, with one point constraint three rotations are, and the normal matrix is
 *              singular (the reference's too).  A pivot of the factorisation that is not finite or not above 1e-12 of its diagonal entry
 *              ends the call with KT_DEFORM_SINGULAR (and KT_OK): the state is the one before that step, steps counts the steps applied.
 *   apply      p' = sum w_i (A_i (p - g_i) + g_i + b_i); n' = normalise(sum w_i A_i^-T n), the old normal kept when that sum is zero or not
 *              finite (so also under a loaded state whose A_i is singular: A_i^-T is then Inf / NaN); double in a fixed order, rounded
 *              to float at the store; colour, curvature and padding untouched.
 * The same input gives the same bytes on every call.  More nodes or constraints than the object was created for: KT_ERR_CAPACITY before
 * any work, nothing written.  n_con = 0 and n = 0 are valid (n_con = 0: KT_DEFORM_INSIGNIFICANT) on an object WITH a graph: every entry but
 * create, destroy and set_graph checks its arguments first (KT_ERR_ARG), then that a graph is set (KT_ERR_STATE, also for n = 0), then the
 * capacity.  max_nodes <= 4096, max_constraints <= 131072 (the per-node constraint lists are built by one lane per node walking them all). */
typedef enum { KT_DEFORM_CONVERGED = 0, KT_DEFORM_MAX_STEPS = 1, KT_DEFORM_INSIGNIFICANT = 2, KT_DEFORM_SINGULAR = 3 } kt_deform_status;
/* null where a kt_deform_params* is taken = the reference's {0.1, 1e-2, 1e-3, 1e-5, 10}; max_steps <= 64 */
typedef struct { double significant_error, delta_tol, error_tol, change_tol; int max_steps, pad; } kt_deform_params;
typedef struct { double error_start, error_end, constraint_error; int steps, status; } kt_deform_result;
typedef struct kt_deform kt_deform;
/* bound to hip_stream (null: the context's stream): every copy and launch goes there */
int kt_deform_create(kt_ctx* ctx, int max_nodes, int max_constraints, void* hip_stream, kt_deform** out);
int kt_deform_destroy(kt_deform* dg);
/* host arrays: node_pos n_nodes x 3 floats, node_time n_nodes.  Resets the state to identity.  n_nodes < 5 or times not increasing: KT_ERR_ARG */
int kt_deform_set_graph(kt_deform* dg, int n_nodes, const float* node_pos, const uint64_t* node_time);
/* host arrays: src_pos n_con x 3 floats, src_time n_con, target n_con x 3 doubles, state_out 12 doubles per node.  The object keeps the state */
int kt_deform_optimise(kt_deform* dg, int n_con, const float* src_pos, const uint64_t* src_time, const double* target, const kt_deform_params* params,
                       double* state_out, kt_deform_result* result);
/* loads a state (12 doubles per node, host): re-applying a saved graph */
int kt_deform_set_state(kt_deform* dg, const double* state);
/* device arrays, 16-byte aligned: n points, n times, idx n x 4, w n x 4.  Asynchronous on the object's stream */
int kt_deform_weights_device(kt_deform* dg, const kt_point_xyzrgbnormal* points_dev, const uint64_t* times_dev, size_t n, int32_t* idx_dev, double* w_dev);
int kt_deform_apply_device(kt_deform* dg, kt_point_xyzrgbnormal* points_dev, const int32_t* idx_dev, const double* w_dev, size_t n);
/* host arrays, in place: upload, weights, apply, download.  Synchronises */
int kt_deform_apply(kt_deform* dg, kt_point_xyzrgbnormal* points, const uint64_t* times, size_t n);
/* The -m mesh (kt_mesh_vertex, 16 bytes) in spans of one time each -- a slab's vertices carry its slice's time (kt_tracker_slice_pose's ts):
 * vertices [span_first[s], span_first[s+1]) carry span_time[s]; span_first: n_spans + 1 host entries, span_first[0] = 0,
 * non-decreasing, span_first[n_spans] = n.  Positions move as kt_deform_apply moves a point at (x, y, z) with that time; rgb untouched.
 * Weights and position in ONE launch (df_apply_mesh): a workgroup does the time search of its span once and keeps the window's nodes and
 * state in LDS.  Spans may be empty.  KT_ERR_ARG with nothing written: a span table that does not start at 0, decreases or does not end
 * at n; null pointers with n > 0; a vertex pointer (either form) that is not 16-byte aligned; n > 2^29 (the mesh stage's own bound).  Then
 * KT_ERR_STATE without a graph.  n = 0 (with any valid table, n_spans = 0 included): KT_OK.  The span table's device copy and the host
 * form's staging (16 bytes per vertex, nothing else) are the object's and grow with the calls.  Two neighbouring slabs carry
 * different times, hence possibly different windows: on an unwelded mesh the two vertices of a seam edge may move apart.  kt_mesh_weld
 * leaves one vertex per seam edge, in the earlier slab's span, and its span_first_out is this call's table. */
int kt_deform_apply_mesh_device(kt_deform* dg, kt_mesh_vertex* vertices_dev, size_t n, const size_t* span_first, const uint64_t* span_time, int n_spans);  /* asynchronous, on the object's stream */
int kt_deform_apply_mesh(kt_deform* dg, kt_mesh_vertex* vertices_host, size_t n, const size_t* span_first, const uint64_t* span_time, int n_spans);       /* upload, apply, download, wait */

/* ---- multi-GPU: independent streams, one tracker per GPU; poses are gathered by the caller's
 * collective (bench.py / the CLI use RCCL all_gather on the buffer filled here) ---- */
/* copies the last k dense poses (k*16 floats, row-major 4x4) into a DEVICE buffer for the gather */
int kt_tracker_export_poses_device(kt_tracker* t, int k, float* dst_dev);

/* The single collective of the path (north star: "a single RCCL gather of per-stream poses over xGMI"; SURVEY 8(b) export list, 8(e)):
 * one process per GPU, rank r owns stream r.  Rank 0 makes the 128-byte RCCL id and hands it to the other ranks out of band
 * (a file for the C++ driver, torch.distributed's store for bench.py); every rank then joins with kt_comm_init.
 * kt_pose_gather: ONE ncclAllGather of k x 16 floats per rank (row-major [R | currentGlobalCamera], the DensePose payload of
 * KintinuousTracker.h:151-169) on the communicator's own stream; all_poses_host receives nranks * k * 16 floats, rank-major. */
#define KT_COMM_ID_BYTES 128
typedef struct kt_comm kt_comm;
int kt_comm_unique_id(unsigned char id[KT_COMM_ID_BYTES]);
int kt_comm_init(kt_ctx* ctx, int rank, int nranks, const unsigned char id[KT_COMM_ID_BYTES], kt_comm** out);
int kt_pose_gather(kt_comm* comm, kt_tracker* t, int k, float* all_poses_host);
int kt_comm_barrier(kt_comm* comm);   /* returns once every rank has called it (a one-float all-gather) */
int kt_comm_destroy(kt_comm* comm);

/* ---- JPEG colour frames: the pixel half of a baseline decode on the device (kt_jpeg.hip) ----
 * The colour payload of a Logger2-style .klg log is a JPEG stream (cvDecodeImage in the reference, utils/RawLogReader.cpp:85, i.e.
 * libjpeg with its defaults).  Its entropy half -- markers, Huffman and run-length decoding, serial within a scan -- runs on the host
 * and leaves quantised coefficients; dequantisation, inverse DCT, upsampling and colour conversion run on the device.  The bytes are
 * those of the host decoder (host/JpegDecoder.h) and of libjpeg.
 *
 * kt_jpeg_layout: the geometry of one image's coefficients.  Component c has blocks_w[c] x blocks_h[c] blocks (whole MCUs) of 64
 * int16 coefficients each, natural (de-zigzagged) order, block-major, not dequantised, starting at coef_offset[c] of one array of
 * n_coef values (components in frame-header order, one right after the other); comp_width / comp_height are libjpeg's
 * downsampled_width / downsampled_height; qt holds the four quantisation tables in natural order (absent ones zero). */
typedef struct {
    int32_t width, height, ncomp, hmax, vmax;
    int32_t h[3], v[3], tq[3], blocks_w[3], blocks_h[3], comp_width[3], comp_height[3];
    uint32_t coef_offset[3];
    uint32_t n_coef;
    uint16_t qt[4][64];
} kt_jpeg_layout;
/* The entropy stage alone, no GPU work (jdmarker.c read_markers + jdhuff.c decode_mcu; kt::jpeg::parseCoefficients of
 * host/JpegDecoder.h): the stream must be a baseline JPEG of exactly width x height.  *n_coef = the number of coefficients; if it
 * exceeds coef_capacity NOTHING is written to layout / coef_host and KT_ERR_CAPACITY is returned.  A stream the decoder rejects
 * returns KT_ERR_ARG with the decoder's message in kt_last_error(), nothing written. */
int kt_host_jpeg_entropy_decode(const uint8_t* data_host, size_t size, int width, int height, kt_jpeg_layout* layout, int16_t* coef_host,
                                size_t coef_capacity, size_t* n_coef);
/* Workspace of the pixel stage (the components' sample planes and a device copy of the coefficients), created once for images of up
 * to max_width x max_height and reusable for any size and sampling below that; bound to hip_stream (null: a stream of its own). */
typedef struct kt_jpeg_ws kt_jpeg_ws;
int kt_jpeg_ws_create(kt_ctx* ctx, int max_width, int max_height, void* hip_stream, kt_jpeg_ws** out);
int kt_jpeg_ws_destroy(kt_jpeg_ws* ws);
void* kt_jpeg_ws_stream(kt_jpeg_ws* ws);
/* makes hip_stream wait (on the device) for everything enqueued on the workspace's stream so far: an event recorded there */
int kt_jpeg_ws_order(kt_jpeg_ws* ws, void* hip_stream);
/* The pixel stage: jpeg_idct_islow (jidctint.c) with dequantisation and the sample_range_limit wrap; h2v1_fancy_upsample /
 * h2v2_fancy_upsample / the replicating upsamplers as jinit_upsampler picks them (jdsample.c); ycc_rgb_convert (jdcolor.c; a grey
 * image: the sample in all three bytes).  coef: n_coef values, a device or (pinned) host pointer; bgr_dev: 3 * width * height dense
 * bytes, 4-byte aligned, B G R per pixel (swap_rb = 0, what cvDecodeImage returns) or R G B (swap_rb = 1).  Enqueues the copy of the
 * coefficients and two kernels on the workspace's stream and returns; one image is in flight per workspace. */
int kt_jpeg_reconstruct(kt_jpeg_ws* ws, const kt_jpeg_layout* layout, const int16_t* coef, int swap_rb, uint8_t* bgr_dev);
/* both stages in one call, then a wait for the workspace's stream (jpeg_read_header .. jpeg_finish_decompress).  A stream the entropy
 * stage rejects returns KT_ERR_ARG before any device work: bgr_dev is not touched. */
int kt_jpeg_decode(kt_jpeg_ws* ws, const uint8_t* data_host, size_t size, int width, int height, int swap_rb, uint8_t* bgr_dev);

#ifdef __cplusplus
}
#endif
#endif /* KT_ABI_H_ */
