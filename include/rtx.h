/*
 * rtx.h — C ABI of librtx.so, the MI355X-native render path of the python-raytracer
 * drop-in (SpacewaIker/python-raytracer @ 2025-02-14).
 *
 * The reference is pure Python, so it has no FFI of its own. Each entry point below
 * replaces one reference interface on the hot path (cited file:line) and is what a
 * ctypes binding of that interface binds:
 *
 *   rtx_scene_create   <- scene_parser.load_scene's object construction
 *                         (provided/scene_parser.py:104-294, geometry ctors in
 *                         provided/geometry/simple_geometry.py:15-18,87-103,180-186,
 *                         provided/geometry/mesh.py:17-70 and
 *                         provided/geometry/hierarchy.py:12-40, textures
 *                         scene_parser.py:222-247): scene objects -> HBM
 *   rtx_camera_set     <- ViewportCamera + the per-frame setup of Scene.render
 *                         (provided/helperclasses.py:69-108, provided/scene.py:36-45)
 *   rtx_render         <- Scene.render's pixel/sample loops + cast_ray + shading
 *                         (provided/scene.py:47-79, :81-116, :140-187, :189-209)
 *   rtx_intersect      <- the Geometry.intersect plugin ABI + closest-hit selection
 *                         (provided/geometry/__init__.py:47-48, provided/scene.py:86-94)
 *   rtx_occluded       <- the Geometry.shadow_intersect plugin ABI + any-hit loop
 *                         (provided/geometry/__init__.py:50-51, provided/scene.py:160-164)
 *   rtx_cast_rays      <- Scene.cast_ray for caller-built rays, batched
 *                         (provided/scene.py:81-116, :140-187, :189-209)
 *   rtx_fb_to_rgb8     <- main.py's rot90 + truncating uint8 conversion
 *                         (provided/main.py:31-33; rot90 is the fb's row order)
 *
 * Conventions
 *   - Every function returns RTX_OK (0) or a negative rtx_status; no C++ exception
 *     crosses the ABI. rtx_last_error() returns a thread-local message for the last
 *     failure on the calling thread.
 *   - Host pointers are read during the call only. Pointers named *_dev are device
 *     (HBM) pointers owned by the caller; the library never frees them.
 *   - rtx_render / rtx_intersect / rtx_occluded / rtx_fb_to_rgb8 are asynchronous on
 *     the given HIP stream (hipStream_t passed as void*; NULL = the default stream).
 *     Scene and camera uploads are synchronous: rtx_camera_set waits for the device to
 *     go idle and copies its tables with a kernel on the null stream, so it must not be
 *     called while any stream is capturing a graph.
 *   - Renders of ONE scene must be stream-ordered (one stream, or events between them):
 *     the hierarchy/texture scenes' split passes keep per-scene scratch (record arrays,
 *     counters, the redo list) that every render of the scene reuses. A render may be
 *     captured into a HIP graph once the scene has rendered eagerly at that size (the
 *     scratch is allocated then); the scene's own buffers live until rtx_scene_destroy.
 *     A captured graph is INVALID after rtx_camera_set: the camera's tables may move and
 *     the kernel it launches was specialized on the old camera (and may be unloaded), so
 *     record it again after every camera upload.
 *   - One device per scene (the current HIP device at rtx_scene_create).
 *   - Numbers carry the reference's types: PyGLM vec3 values are float (fp32), Python
 *     scalars are double (fp64).
 */
#ifndef RTX_H
#define RTX_H

#if !defined(__HIPCC_RTC__)
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_ABI_VERSION 6

typedef enum rtx_status {
    RTX_OK = 0,
    RTX_ERR_INVALID = -1,     /* bad argument / inconsistent description */
    RTX_ERR_HIP = -2,         /* HIP runtime error (message in rtx_last_error) */
    RTX_ERR_UNSUPPORTED = -3, /* feature not built (e.g. textures, hierarchy nodes) */
    RTX_ERR_STATE = -4        /* e.g. rtx_render before rtx_camera_set */
} rtx_status;

typedef enum rtx_object_type { RTX_SPHERE = 0, RTX_PLANE = 1, RTX_BOX = 2, RTX_MESH = 3, RTX_NODE = 4 } rtx_object_type;
typedef enum rtx_hierarchy_type {
    RTX_UNION = 0, RTX_INTERSECTION = 1, RTX_DIFFERENCE = 2, RTX_HIER_OTHER = 3  /* other: no hits */
} rtx_hierarchy_type;
typedef enum rtx_material_type { RTX_MAT_DIFFUSE = 0, RTX_MAT_MIRROR = 1, RTX_MAT_REFRACTIVE = 2 } rtx_material_type;
typedef enum rtx_light_type { RTX_LIGHT_POINT = 0, RTX_LIGHT_DIRECTIONAL = 1 } rtx_light_type;
typedef enum rtx_bv_type { RTX_BV_AABB = 0, RTX_BV_SPHERE = 1 } rtx_bv_type;
typedef enum rtx_jitter_mode { RTX_JITTER_OFF = 0, RTX_JITTER_PHILOX = 1, RTX_JITTER_REPLAY = 2 } rtx_jitter_mode;

/* One geometry record. Top-level objects (parent == -1) are in scene (JSON) order, which
 * is the closest-hit tie break (min() keeps the first minimum, provided/scene.py:94).
 * Hierarchy nodes (RTX_NODE, provided/geometry/hierarchy.py) are followed by their
 * subtree in preorder: every record after a node whose parent is that node is one of
 * its children, in child order. Child records carry what the parser gives them:
 * materials after Hierarchy.set_fallback_material (hierarchy.py:21-28), speeds after
 * traverse_children's `speed + child speed` (scene_parser.py:268-271). */
typedef struct rtx_object {
    int32_t type;          /* rtx_object_type */
    int32_t n_mats;        /* associated materials (Plane: 1 = plain, >=2 = checker) */
    int32_t mat[2];        /* material indices; mat[0] for sphere / box / mesh */
    int32_t has_speed;     /* 0 = speed None; else position + speed * time */
    float speed[3];
    float a[3];            /* sphere centre | plane point | box minpos | (mesh unused) */
    float b[3];            /* plane normal  | box maxpos */
    double radius;         /* sphere radius (Python float) */
    int32_t tri_begin;     /* mesh: first triangle in rtx_scene_desc.triangles */
    int32_t tri_count;     /* mesh: number of triangles (faces in OBJ order) */
    int32_t bv_type;       /* mesh: rtx_bv_type chosen by Mesh.__init__ (mesh.py:44-51) */
    int32_t flat;          /* mesh: flat_shaded */
    float bv_a[3];         /* mesh BV: AABB min | sphere centre */
    float bv_b[3];         /* mesh BV: AABB max */
    double bv_radius;      /* mesh BV: sphere radius (Python float) */
    int32_t parent;        /* -1: top-level; else index of the enclosing RTX_NODE record */
    int32_t hierarchy_type;/* node: rtx_hierarchy_type */
    float trs[9];          /* node: position, rotation (degrees), scale (Hierarchy.make_matrices) */
    int32_t texture;       /* plane / box: index into rtx_scene_desc.textures, -1 = none */
    double texture_scale;  /* plane: texture_scale (scene_parser.py:226, default 1.0) */
} rtx_object;

/* A texture as Image.getpixel sees it (scene_parser.py:224, simple_geometry.py:168):
 * rgb[3 * (j * width + i) + c] = getpixel((i, j))[c]. */
typedef struct rtx_texture {
    int32_t width, height;
    const uint8_t* rgb;
} rtx_texture;

/* One mesh face after Mesh.__init__'s (v + translate) * scale transform (mesh.py:24),
 * with the per-vertex smooth normals of _compute_normals (mesh.py:53-70; ignored
 * when the mesh is flat shaded). */
typedef struct rtx_triangle {
    float v0[3], v1[3], v2[3];
    float n0[3], n1[3], n2[3];
} rtx_triangle;

typedef struct rtx_material {
    float diffuse[3];
    float specular[3];
    double hardness;       /* Python number; `x ** hardness` in fp64 */
    int32_t type;          /* rtx_material_type */
    double tint;
    double refr_index;
} rtx_material;

typedef struct rtx_light {
    int32_t type;          /* rtx_light_type */
    float colour[3];
    float vector[3];       /* position (point) | direction (directional) */
    double power;          /* directional lights: 1.0 (scene_parser.py:116-118) */
} rtx_light;

typedef struct rtx_scene_desc {
    int32_t n_objects;
    const rtx_object* objects;
    int32_t n_materials;
    const rtx_material* materials;
    int32_t n_lights;
    const rtx_light* lights;
    int32_t n_triangles;
    const rtx_triangle* triangles;
    float ambient[3];
    int32_t n_textures;
    const rtx_texture* textures;
} rtx_scene_desc;

/* Per-frame camera state. Tables are the reference's scalar sequences, evaluated on the
 * host exactly as provided/scene.py computes them. */
typedef struct rtx_camera_desc {
    int32_t width, height;   /* full image size */
    int32_t col0, ncols;     /* rendered column strip (np.array_split range of Scene.render) */
    const float* xs;         /* [ncols] fp32 of the fp64 x running sum (scene.py:42,77) */
    const float* ys;         /* [height] fp32 of the fp64 y running sum, bottom row first (scene.py:48,75) */
    float position[3];
    float u[3], v[3], w[3];
    double d;                /* ViewportCamera.d (1.0) */
    double focal_length;
    int32_t n_dof, n_aa;
    const float* dof_origins;/* [n_dof][3] _sunflower_spread(dof, position, aperture) */
    const float* aa_origins; /* [n_dof][n_aa][3] _sunflower_spread(aa, dof_origin, 2(dx+dy)) */
    int32_t n_times;         /* motion times per frame (the divisor's factor) */
    const double* times;     /* [n_times] ViewportCamera.motion_times; [n_frames][n_times] for a sequence */
    int32_t jitter;          /* rtx_jitter_mode */
    double jitter_scale;     /* 0.1 * (dx + dy) (scene.py:64) */
    uint64_t seed;           /* RTX_JITTER_PHILOX key */
    const float* noise;      /* RTX_JITTER_REPLAY: host [ncols][height][n_dof][n_aa][3] values of
                                np.random.rand() in the reference's call order (i, j, dof, aa) */
    int32_t n_frames;        /* frame sequence (no reference counterpart): 0 or 1 = one window of motion
                                times, as above; F > 1 (<= 65535, F * n_times <= 2^24) = F windows of
                                n_times each, which rtx_render_sequence renders by index. Every other
                                render call uses window 0. Times must be finite. */
} rtx_camera_desc;

/* Device counters written by rtx_render when counters_dev != NULL (uint64[RTX_COUNTERS]). */
#define RTX_COUNTERS 16
#define RTX_CNT_CAST0 0      /* [0..9]: cast_ray calls that intersect, by recursion depth */
#define RTX_CNT_SHADOW 10    /* shadow rays */
#define RTX_CNT_SHADE 11     /* _compute_regular_lighting calls */
#define RTX_CNT_TRI 12       /* ray-triangle tests */

typedef struct rtx_scene rtx_scene;

int rtx_abi_version(void);
const char* rtx_last_error(void);

int rtx_scene_create(const rtx_scene_desc* desc, rtx_scene** out);
int rtx_scene_destroy(rtx_scene* scene);
int rtx_camera_set(rtx_scene* scene, const rtx_camera_desc* cam);

/* Renders image rows [row0, row0 + nrows) (row 0 = top of the PNG) of the camera's
 * column strip into fb_dev: float32 [nrows][ncols][3], i.e. the reference image
 * rotated by main.py's rot90. */
int rtx_render(rtx_scene* scene, int32_t row0, int32_t nrows, float* fb_dev,
               uint64_t* counters_dev, void* hip_stream);

/* Multi-GPU load balance (no reference counterpart: the reference splits columns across
 * processes, provided/scene.py:36-37 + render.nu): renders the 8-row groups phase,
 * phase + stride, phase + 2 stride, ... of the image (row 0 = top), packed in order into
 * fb_dev: float32 [rtx_group_rows(height, phase, stride)][ncols][3]. Rank r of N calls
 * it with (r, N), so every rank gets rows from the whole frame (sky and ground alike).
 * Pixel values equal rtx_render's for the same rows. */
int rtx_render_groups(rtx_scene* scene, int32_t phase, int32_t stride, float* fb_dev,
                      uint64_t* counters_dev, void* hip_stream);

/* rtx_render / rtx_render_groups with main.py's PNG conversion fused into the render
 * (provided/main.py:31-33): out_dev receives uint8 [rows][ncols][3] = (v * 255.0) truncated
 * of the fp32 values rtx_render would write — identical bytes to rtx_render followed by
 * rtx_fb_to_rgb8, with 4x fewer bytes stored (and gathered, across ranks). */
int rtx_render_rgb8(rtx_scene* scene, int32_t row0, int32_t nrows, uint8_t* out_dev,
                    uint64_t* counters_dev, void* hip_stream);
int rtx_render_groups_rgb8(rtx_scene* scene, int32_t phase, int32_t stride, uint8_t* out_dev,
                           uint64_t* counters_dev, void* hip_stream);

/* Frames of one scene state in ONE launch (no reference counterpart: a launch-count
 * optimisation of the multi-GPU frame loop, rtx.distributed.FrameExchange): nframes
 * copies of rtx_render (rgb8 = 0: fp32) / rtx_render_rgb8 (rgb8 != 0) of rows
 * [row0, row0 + nrows), frame f at out_dev + f * frame_stride_bytes (>= one frame's
 * bytes; a multiple of 4 for fp32). gridDim.y = nframes fills the GPU that one
 * 1/N-of-a-frame launch per rank leaves partly idle at N = 8. 1 <= nframes <= 65535. */
int rtx_render_frames(rtx_scene* scene, int32_t row0, int32_t nrows, void* out_dev, int32_t rgb8, int32_t nframes,
                      int64_t frame_stride_bytes, uint64_t* counters_dev, void* hip_stream);
/* The same for rtx_render_groups / rtx_render_groups_rgb8 (interleaved 8-row groups). */
int rtx_render_groups_frames(rtx_scene* scene, int32_t phase, int32_t stride, void* out_dev, int32_t rgb8,
                             int32_t nframes, int64_t frame_stride_bytes, uint64_t* counters_dev, void* hip_stream);

/* Frames [frame0, frame0 + nframes) of the camera's sequence (rtx_camera_desc.n_frames windows
 * of n_times motion times; no reference counterpart) in ONE launch: slot k of out_dev (at
 * out_dev + k * frame_stride_bytes, as rtx_render_frames) receives what rtx_render /
 * rtx_render_rgb8 writes for a camera whose motion times are window frame0 + k -- the same
 * fp32 sums in the same order, divided by n_dof * n_aa * n_times. A moving scene's frames
 * therefore cost one camera upload, not one each. RTX_ERR_INVALID for a frame range outside
 * the sequence; the stride rules are rtx_render_frames'. counters_dev accumulates over all
 * the frames. The culling structures of a sequence camera cover the time range of all its
 * windows, so a long sequence may render faster in several shorter ones. */
int rtx_render_sequence(rtx_scene* scene, int32_t row0, int32_t nrows, void* out_dev, int32_t rgb8, int32_t frame0,
                        int32_t nframes, int64_t frame_stride_bytes, uint64_t* counters_dev, void* hip_stream);
/* The same for rtx_render_groups / rtx_render_groups_rgb8 (interleaved 8-row groups). */
int rtx_render_groups_sequence(rtx_scene* scene, int32_t phase, int32_t stride, void* out_dev, int32_t rgb8,
                               int32_t frame0, int32_t nframes, int64_t frame_stride_bytes, uint64_t* counters_dev,
                               void* hip_stream);

/* First-hit feature buffers of rows [row0, row0 + nrows) of the strip (no reference
 * counterpart): what the FIRST sample of each pixel sees -- the ray of DOF origin 0 and AA
 * origin 0 (provided/scene.py:57-61) with that sample's jitter draw (:63-65, the draw
 * rtx_render uses for it), at the first motion time of window `frame` (0 for a camera
 * without a sequence). Buffers are pixel-major with row 0 at the top, like the framebuffer;
 * each may be NULL (not written), but not all six:
 *   depth    f32 [nrows][ncols]     fp32 rounding of first_intersect.time (scene.py:86-94), +inf on a miss
 *   normal   f32 [nrows][ncols][3]  first_intersect.normal as the reference has it (not renormalised), 0
 *   position f32 [nrows][ncols][3]  first_intersect.position, 0
 *   albedo   f32 [nrows][ncols][3]  the `diffuse` of _compute_regular_lighting (scene.py:143-146): get_diffuse
 *                                   of planes and boxes (checkers, textures; also inside hierarchies), else the
 *                                   material's diffuse, whatever the material's type; 0
 *   object   i32 [nrows][ncols]     index of the hit's top-level object (as rtx_intersect), -1
 *   material i32 [nrows][ncols]     index of first_intersect.mat (as rtx_intersect), -1
 * Every value is bit-identical to the reference's for that ray. Asynchronous on the stream.
 * RTX_ERR_STATE before rtx_camera_set; RTX_ERR_INVALID for a null scene, a row range outside
 * the image, six null pointers or a frame outside the camera's sequence; the arguments are
 * checked before any HIP call. rtx_last_kernel is left as it is. */
int rtx_render_aov(rtx_scene* scene, int32_t row0, int32_t nrows, int32_t frame, float* depth_dev, float* normal_dev,
                   float* position_dev, float* albedo_dev, int32_t* object_dev, int32_t* material_dev,
                   void* hip_stream);

/* Occlusion buffers of rows [row0, row0 + nrows) of the strip (no reference counterpart): the
 * visibility the reference computes per shadow ray and multiplies away (provided/scene.py:
 * 148-167), kept, plus ambient occlusion. The ray, the first hit and the motion time t are
 * rtx_render_aov's (DOF origin 0, AA origin 0, that sample's jitter draw, the first motion
 * time of window `frame`); p and n below are the `position` and `normal` it writes. Buffers
 * are pixel-major with row 0 at the top; each may be NULL (not written), but not both:
 *   lights  u32 [nrows][ncols]  bit i set iff light i's shadow ray from p is NOT occluded at
 *                               time t (scene.py:150-167, skip == False): a point light's has
 *                               origin p, direction light.vector - p (one fp32 subtraction per
 *                               component) and t_max 1.0, a directional light's origin p,
 *                               direction -light.vector and t_max +inf. Pure visibility: the
 *                               bit does not look at which way n faces. What rtx_occluded
 *                               answers for that ray. 0 on a miss. A scene with more than 32
 *                               lights gets RTX_ERR_INVALID when this buffer is requested.
 *   ao      f32 [nrows][ncols]  fl32(u) / fl32(n_dirs), u the number of the n_dirs rays that
 *                               rtx_occluded reports free; 1.0 on a miss. Ray k starts at p
 *                               (no offset, like the reference's shadow rays; the epsilons of
 *                               shadow_intersect apply), is cast at time t with t_max
 *                               ao_radius, and runs along d_k below.
 * ao_dirs is a host array of n_dirs local directions [n_dirs][3] (x, y, z), 1 <= n_dirs <=
 * RTX_AO_MAX_DIRS, all finite, z along the normal; it is read during the call and passed to the
 * kernel by value. They are used as given (not normalised; a z < 0 points below the surface).
 * The frame is built in unfused fp32 in exactly this order:
 *   n^ = normalize(n)            (glm normalize: n * (1 / sqrt(dot(n, n))))
 *   s = copysignf(1, n^.z);  a = -1 / (s + n^.z);  b = (n^.x * n^.y) * a
 *   T = (1 + ((s * n^.x) * n^.x) * a,  s * b,  -(s * n^.x))
 *   U = (b,  s + ((n^.y * n^.y) * a),  -n^.y)
 *   d_k = ((x_k * T) + (y_k * U)) + (z_k * n^)      per component
 * The hemisphere is about the STORED normal: it is not flipped toward the viewer, so a surface
 * seen from behind (the inside of a sphere, a plane from below) sends its rays away from the
 * camera's side. A hit whose normal has zero length is outside the contract. ao_radius is
 * > 0 or +inf. ao_dirs, n_dirs and ao_radius are ignored when ao_dev is NULL.
 * Both answers are bit-identical to the reference's shadow_intersect loop for those rays.
 * Asynchronous on the stream; the stream-ordering and graph-capture rules are rtx_render_aov's.
 * RTX_ERR_STATE before rtx_camera_set; RTX_ERR_INVALID for a null scene, a row range outside
 * the image, two null buffers, a frame outside the camera's sequence, `lights` on a scene with
 * more than 32 lights, and with ao_dev: null ao_dirs, n_dirs outside [1, RTX_AO_MAX_DIRS], a
 * non-finite direction component, an ao_radius that is NaN or <= 0. The arguments are checked
 * before any HIP call. rtx_last_kernel is left as it is. */
#define RTX_AO_MAX_DIRS 64
int rtx_render_occlusion(rtx_scene* scene, int32_t row0, int32_t nrows, int32_t frame, uint32_t* lights_dev,
                         float* ao_dev, const float* ao_dirs, int32_t n_dirs, double ao_radius, void* hip_stream);

/* Resolved feature buffers of rows [row0, row0 + nrows) of the strip (no reference counterpart):
 * what each pixel covers over ALL its samples, so the buffers line up with the colour rtx_render
 * stores for any camera (depth of field, motion blur, antialiasing), where rtx_render_aov
 * describes the first sample only. The pixel's samples are visited as the render visits them
 * (provided/scene.py:57-69): kd over the n_dof DOF origins, ka over the n_aa AA origins, kt over
 * the n_times motion times of window `frame` (0 for a camera without a sequence), time fastest.
 * Sample (kd, ka) has the origin and direction of the render's sample, with the jitter draw the
 * render uses for it (scene.py:63-65); each of the S = n_dof * n_aa * n_times samples is
 * intersected with the scene (first_intersect, scene.py:86-94). H is the number of samples that
 * hit. Buffers are pixel-major with row 0 at the top; each may be NULL (not written), but not
 * all five:
 *   alpha   f32 [nrows][ncols]     fl32(H) / fl32(S): the pixel's coverage
 *   matte   f32 [nrows][ncols]     fl32(M) / fl32(S), M the number of samples whose first hit's
 *                                  top-level object (rtx_render_aov's `object`) is in matte_objects
 *   depth   f32 [nrows][ncols]     (sum over the hit samples of rtx_render_aov's depth) / fl32(H);
 *                                  +inf when H == 0. A mean over the hits.
 *   normal  f32 [nrows][ncols][3]  (sum over the hit samples of rtx_render_aov's normal, not
 *                                  renormalised) / fl32(S)
 *   albedo  f32 [nrows][ncols][3]  (sum over the hit samples of rtx_render_aov's albedo) / fl32(S)
 * normal and albedo are means over all S samples: a miss adds nothing, so they are premultiplied
 * by the coverage like the colour, whose misses add black. Every sum is fp32, starts at +0 and
 * is added in sample order; every division is one correctly rounded fp32 division. Each
 * sample's values are bit-identical to the reference's for its ray. For a one-sample camera
 * every buffer equals rtx_render_aov's as a value (a -0 component is +0 after the sum) and
 * alpha is 1 where `object` >= 0.
 * matte_objects is a host array of n_matte >= 1 indices of top-level objects, each in
 * [0, n_objects) and below RTX_MATTE_MAX_OBJECTS; duplicates are allowed. It is read during the
 * call and passed to the kernel by value as a bit set; both are ignored when matte_dev is NULL.
 * Asynchronous on the stream; the stream-ordering and graph-capture rules are rtx_render_aov's.
 * RTX_ERR_STATE before rtx_camera_set; RTX_ERR_INVALID for a null scene, a row range outside the
 * image, five null buffers, a frame outside the camera's sequence, and with matte_dev: null
 * matte_objects, n_matte < 1 or an index out of range; RTX_ERR_UNSUPPORTED for a scene with
 * hierarchies or textures (this pass is built for flat scenes only). The arguments are checked
 * before any HIP call. rtx_last_kernel is left as it is. */
#define RTX_MATTE_MAX_OBJECTS 256
int rtx_render_resolved(rtx_scene* scene, int32_t row0, int32_t nrows, int32_t frame, float* alpha_dev,
                        float* matte_dev, float* depth_dev, float* normal_dev, float* albedo_dev,
                        const int32_t* matte_objects, int32_t n_matte, void* hip_stream);

/* Ranked id-coverage buffers of rows [row0, row0 + nrows) of the strip (no reference
 * counterpart): per pixel, the objects or materials that cover the most samples, with their
 * exact sample counts, so that the matte of ANY object set is a lookup after one pass
 * (Cryptomatte-style). Rows, strip, `frame`, the sample order (kd over the DOF origins, ka over
 * the AA origins, kt over the window's motion times, time fastest), the rays and the jitter
 * draws (for Philox jitter the block of the pair (kd * n_aa + ka) >> 1, the odd sample keeping
 * its pair's uniforms) are rtx_render_resolved's. Each sample that hits has a key:
 *   RTX_ID_OBJECT    rtx_render_aov's `object`, the first hit's top-level object
 *   RTX_ID_MATERIAL  rtx_render_aov's `material` (a checkered plane has two)
 * Per pixel a table of RTX_ID_SLOTS slots starts empty. A miss does nothing. A hit with key k:
 * a slot that holds k counts one more; else the lowest-numbered empty slot becomes (k, 1); else
 * `dropped` counts one more. So the table keeps the first RTX_ID_SLOTS distinct keys in sample
 * order, with exact counts. After the last sample the filled slots are ranked by count
 * descending, equal counts by key ascending; empty slots come last. Buffers are pixel-major
 * with row 0 at the top; each may be NULL (not written), but not all three:
 *   ids     i32 [nrows][ncols][ranks]  the key of rank r; -1 for an empty rank
 *   counts  i32 [nrows][ncols][ranks]  the count of rank r; 0 for an empty rank
 *   other   i32 [nrows][ncols]         dropped + the counts of the ranks >= `ranks`, which are
 *                                      not written
 * Hence sum(counts) + other == H, rtx_render_resolved's hit count, and where other == 0 the
 * written ranks are the pixel's complete and exact id histogram: with S = n_dof * n_aa *
 * n_times, fl32(sum of the counts whose id is in a set) / fl32(S) is rtx_render_resolved's
 * `matte` of that set, bit for bit. Counts are integers, not coverages, to keep that exact.
 * 1 <= ranks <= RTX_ID_SLOTS.
 * Asynchronous on the stream; the stream-ordering and graph-capture rules are rtx_render_aov's.
 * RTX_ERR_STATE before rtx_camera_set; RTX_ERR_INVALID for a null scene, a row range outside the
 * image, three null buffers, a frame outside the camera's sequence, a `key` that is neither of
 * the two values, ranks outside [1, RTX_ID_SLOTS]; RTX_ERR_UNSUPPORTED for a scene with
 * hierarchies or textures (a flat-scene pass, as rtx_render_resolved is). nrows == 0 is RTX_OK
 * and launches nothing. The arguments are checked before any HIP call. rtx_last_kernel is left
 * as it is. */
#define RTX_ID_SLOTS 8
typedef enum rtx_id_key { RTX_ID_OBJECT = 0, RTX_ID_MATERIAL = 1 } rtx_id_key;
int rtx_render_ids(rtx_scene* scene, int32_t row0, int32_t nrows, int32_t frame, int32_t key, int32_t ranks,
                   int32_t* ids_dev, int32_t* counts_dev, int32_t* other_dev, void* hip_stream);

/* Light groups of rows [row0, row0 + nrows) of the strip (no reference counterpart): the colour
 * rtx_render stores, separated by light set, in one pass. out_dev is f32
 * [n_groups][nrows][ncols][3]; each plane has the framebuffer's layout (row 0 at the top), so
 * rtx_fb_to_rgb8 applies to a plane. Plane g holds, bit for bit, what rtx_render stores for
 * those rows with the motion times of window `frame` (0 for a camera without a sequence) for the
 * scene with two changes: its lights are exactly those with light_group[li] == g, in their
 * original order, and its ambient is the scene's when ambient_group == g, else (0, 0, 0).
 * Everything else is rtx_render's: the samples and their order (DOF origins, AA origins, motion
 * times, time fastest), the jitter draws, the per-level clamp of provided/scene.py:113-115, the
 * fp32 sums from +0 and the one division by fl32(S) per channel.
 *   light_group    host array of n_lights entries, read during the call and passed to the kernel
 *                  by value: the group of light li in [0, n_groups), or -1 for a light that
 *                  belongs to no group and lights nothing (its shadow rays are not traced).
 *   n_groups       1 <= n_groups <= RTX_LIGHT_GROUPS_MAX. A group may be empty: its plane is
 *                  black, or the ambient term alone.
 *   ambient_group  the group that receives the scene's ambient term, or -1 for none.
 * Every ray chain is traced once and every light's shadow ray once per chain level, whatever
 * the grouping (no ray of the renderer depends on a light); only the shading is per group.
 * With n_groups == 1, every light in group 0 and ambient_group == 0 the plane equals
 * rtx_render's framebuffer bit for bit. The planes are clamped per chain level, as the
 * reference clamps: their sum equals the beauty image only where no clamp engages, and then
 * only up to fp32 rounding -- the sum is documented, not guaranteed.
 * Asynchronous on the stream; the stream-ordering and graph-capture rules are rtx_render_aov's.
 * RTX_ERR_STATE before rtx_camera_set; RTX_ERR_INVALID for a null scene, a row range outside the
 * image, a null out_dev, a frame outside the camera's sequence, a null light_group, n_groups
 * outside [1, RTX_LIGHT_GROUPS_MAX], a scene with more than 32 lights, a light_group entry or
 * ambient_group outside [-1, n_groups); RTX_ERR_UNSUPPORTED for a scene with hierarchies or
 * textures (a flat-scene pass, as rtx_render_resolved is). nrows == 0 is RTX_OK and launches
 * nothing; a scene without lights is valid. The arguments are checked before any HIP call.
 * rtx_last_kernel is left as it is; the call writes no counters. */
#define RTX_LIGHT_GROUPS_MAX 8
int rtx_render_light_groups(rtx_scene* scene, int32_t row0, int32_t nrows, int32_t frame, const int32_t* light_group,
                            int32_t n_groups, int32_t ambient_group, float* out_dev, void* hip_stream);

/* Rows rtx_render_groups writes for an image of `height` rows (-1: bad arguments). */
int32_t rtx_group_rows(int32_t height, int32_t phase, int32_t stride);

/* Closest hit of n rays (SoA device arrays ray_o_dev/ray_d_dev = [3][n] fp32) at one
 * motion time. Outputs: t (fp64, +inf on miss), object index (-1), material index (-1),
 * normal [3][n], position [3][n]. Any output pointer may be NULL. */
int rtx_intersect(rtx_scene* scene, int64_t n, const float* ray_o_dev, const float* ray_d_dev,
                  double time, double* t_dev, int32_t* obj_dev, int32_t* mat_dev,
                  float* normal_dev, float* position_dev, void* hip_stream);

/* Any-hit shadow test of n rays against every object with per-ray t_max (fp64). */
int rtx_occluded(rtx_scene* scene, int64_t n, const float* ray_o_dev, const float* ray_d_dev,
                 const double* t_max_dev, double time, uint8_t* occluded_dev, void* hip_stream);

/* Colours of caller-built rays: Scene.cast_ray (provided/scene.py:81-116 -- closest hit, shadow
 * rays, lighting, the reflect / refract chain of up to 10 casts, the per-level clamp) as a
 * batched call; with rtx_intersect and rtx_occluded the third entry of the plugin ABI. For a
 * camera the reference lacks (panorama, orthographic, a probe at a surface point), a moving
 * camera without a camera upload per frame, a reflection pass from rtx_render_aov's position /
 * normal buffers. Works before rtx_camera_set, like rtx_intersect, and uses nothing of the
 * camera: none of its bins, shadow bins or self-test tables, which hold for its own rays only.
 *   ray_o_dev, ray_d_dev  n rays, SoA fp32 [3][n] (rtx_intersect's layout). Directions are used
 *                         as given: the reference does not normalise them (scene.py:176's half
 *                         vector reads the ray's own direction).
 *   times                 host array of n_times motion times, 1 <= n_times <= RTX_CAST_MAX_TIMES,
 *                         each finite; cast to fp32 like a camera's. Every ray is cast at every
 *                         time, with the same origin and direction.
 *   group                 rays per output colour, >= 1 and a divisor of n (group * n_times
 *                         below 2^31).
 *   rgb_dev               fp32 [n / group][3], pixel-major like the framebuffer (rtx_fb_to_rgb8
 *                         applies). rgb[j] = (c_0 + c_1 + ... + c_{S-1}) / fl32(S), S = group *
 *                         n_times, where c_s is the clamped fp32 colour of ray j * group +
 *                         s / n_times at times[s % n_times] (time fastest: the loop nest of one
 *                         pixel, scene.py:57-69), added in that order in fp32 from +0 and divided
 *                         once, correctly rounded: what rtx_render stores for a pixel whose
 *                         samples are these rays. Every c_s is bit-identical to the reference's.
 *   counters_dev          NULL, or RTX_COUNTERS tallies in rtx_render's layout, accumulated.
 * Asynchronous on the stream. A scene with hierarchy nodes gets their boxes for
 * [min(times), max(times)] uploaded in stream order by the call (as rtx_intersect does for its
 * one time), so calls on one scene must be stream-ordered, and only a scene without hierarchy
 * nodes may have the call captured into a HIP graph. RTX_ERR_INVALID for a null scene, n < 0,
 * null rays or a null output with n > 0, group < 1 or not a divisor of n, n_times outside
 * [1, RTX_CAST_MAX_TIMES] or null times, a non-finite time (as fp32), group * n_times >= 2^31,
 * or more than 2^31 - 1 blocks; all checked before any HIP call. RTX_ERR_STATE when the scene
 * lives on another device than the current one. n == 0 is RTX_OK and launches nothing.
 * rtx_last_kernel is left as it is. */
#define RTX_CAST_MAX_TIMES 64
int rtx_cast_rays(rtx_scene* scene, int64_t n, const float* ray_o_dev, const float* ray_d_dev,
                  const double* times, int32_t n_times, int32_t group, float* rgb_dev,
                  unsigned long long* counters_dev, void* hip_stream);

/* out_dev[i] = (uint8)(fb_dev[i] * 255.0) in fp64 with truncation (main.py:33). */
int rtx_fb_to_rgb8(const float* fb_dev, uint8_t* out_dev, int64_t n_values, void* hip_stream);

/* Observability (no reference counterpart): the name of the kernel the last
 * rtx_render / rtx_render_groups call on this scene launched — "rtx_jit_render_<flags>"
 * for a scene-specialized (hiprtc) kernel, "k_render_<flags>" / "k_render_ext_<flags>"
 * for the precompiled generic ones; "" before the first render. Valid until the next
 * render call on the scene or rtx_scene_destroy. */
const char* rtx_last_kernel(const rtx_scene* scene);

/* Observability (no reference counterpart): the number of scene-specialized kernel
 * modules loaded in this process. Kernels whose source carries one scene's record values
 * are unloaded once no scene holds them and more than jit_idle_baked (option, default 8)
 * such idle modules exist, so the count stays bounded as scenes come and go. */
int32_t rtx_jit_modules(void);

/* Library options (no reference counterpart; INTEGRATION.md "Options"): process-wide
 * switches of the culling structures, the split hierarchy passes, the scene-specialized
 * kernels and their caches, by name ("split", "bins", "jit", "uniform_hit", ...). Each starts from
 * $RTX_<NAME> when that is set in the environment, else from its default; set them before
 * rendering (they are read per render / per camera upload, not synchronised with renders
 * on other threads). Values are text: a number, or a string for "jit_cache" / "jit_flags".
 * RTX_ERR_INVALID for an unknown name or a malformed number. */
int rtx_set_option(const char* name, const char* value);
/* The option's current value as text into value[cap] (RTX_ERR_INVALID if it does not fit). */
int rtx_get_option(const char* name, char* value, int32_t cap);
/* Name of option i (0, 1, ...; NULL past the last). */
const char* rtx_option_name(int32_t i);

/* Scene-specialized kernels compiled on a host thread (option jit_async, default 1; no
 * reference counterpart): a scene's first renders launch the precompiled generic kernel,
 * which renders the same bytes, while hiprtc compiles the specialized one; a later render
 * that finds the compile done switches to it. rtx_jit_wait picks up the scene's finished
 * compiles -- block != 0: waits for all of them first -- and returns how many are still
 * compiling (0 once every kernel the scene's camera has rendered with is resolved). */
int32_t rtx_jit_wait(rtx_scene* scene, int32_t block);

/* Multi-GPU frame loop (no reference counterpart; the reference's strip renders and glue,
 * render.nu:10-15 + provided/glue.py:17-27, as one HIP graph per frame): launches the
 * instantiated graph graph_exec (a hipGraphExec_t, e.g. one rank's render + RCCL gather of
 * a frame captured by rtx.distributed.FrameGraph) n times in order on hip_stream, from C,
 * so a frame costs one hipGraphLaunch of host time. Asynchronous; RTX_ERR_INVALID for a
 * null graph or n < 0. */
int rtx_graph_launch(void* graph_exec, int32_t n, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* RTX_H */
