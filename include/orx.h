/*
 * orx.h — C ABI of the MI355X-native render core (liborx.so).
 *
 * This is the drop-in boundary for ico-eagleye/OppositeRenderer's
 * `OptixRenderer` (RenderEngine/renderer/OptixRenderer.h:21-43) and the
 * parts of `IScene` (RenderEngine/scene/IScene.h:16-29) that the renderer
 * consumes.  Plain pointers and sizes only; no C++ or torch types cross it.
 * Errors never throw: every call returns an orx_status and the message of
 * the last failure is kept per renderer (orx_last_error), replacing the
 * reference's std::exception(const char*) (OptixRenderer.cpp:816-820).
 *
 * Reference entry point -> orx call
 *   OptixRenderer::OptixRenderer() + initialize(ComputeDevice)
 *       (OptixRenderer.cpp:81-104, :113-400)              -> orx_create
 *   OptixRenderer::initScene(IScene&) (:436-485)          -> orx_init_scene
 *   OptixRenderer::renderNextIteration(...) (:507-821)    -> orx_render_next_iteration
 *   OptixRenderer::getOutputBuffer(void*) (:860-865)      -> orx_get_output
 *   getWidth/getHeight/getScreenBufferSizeBytes (:850-870)-> orx_width/orx_height/orx_output_bytes
 *   OptixRenderer::EMITTED_PHOTONS_PER_ITERATION (.h:43)  -> orx_emitted_photons_per_iteration
 *   ~OptixRenderer() (:106-111)                           -> orx_destroy
 */
#ifndef ORX_H
#define ORX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORX_ABI_VERSION 1u

typedef struct orx_renderer orx_renderer;

typedef enum {
    ORX_OK = 0,
    ORX_ERR_INVALID_ARGUMENT = 1,
    ORX_ERR_STATE = 2,          /* e.g. initScene before initialize, render before initScene */
    ORX_ERR_DEVICE = 3,         /* HIP runtime failure */
    ORX_ERR_NO_LIGHTS = 4,      /* "No lights exists in this scene." (OptixRenderer.cpp:444-447) */
    ORX_ERR_GRID_TOO_LARGE = 5, /* "Too many cells in SpatialHash.cu" (OptixRenderer_SpatialHash.cu:243-247) */
    ORX_ERR_OUT_OF_MEMORY = 6,
    ORX_ERR_UNSUPPORTED = 7
} orx_status;

/* RenderMethod::E order (RenderEngine/renderer/RenderMethod.h:13-19). */
typedef enum {
    ORX_METHOD_PATH_TRACING = 0,
    ORX_METHOD_VCM_BIDIRECTIONAL_PATH_TRACING = 1,
    ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING = 2
} orx_method;

/* Camera inputs (Camera.h:72-79).  The engine derives lookdir / camera_u /
 * camera_v exactly as Camera::setup (Camera.cpp:333-345). */
typedef struct {
    float eye[3];
    float lookat[3];
    float up[3];
    float hfov;     /* degrees */
    float vfov;     /* degrees */
    float aperture; /* > 0 enables thin-lens depth of field (helpers/camera.h:11-27) */
} orx_camera;

/* RenderServerRenderRequestDetails (clientserver/RenderServerRenderRequestDetails.h:15-33). */
typedef struct {
    orx_camera camera;
    int32_t method;  /* orx_method */
    uint32_t width;
    uint32_t height;
    double ppm_alpha;
} orx_request;

/* Material classes of RenderEngine/material (one per .cpp). */
typedef enum {
    ORX_MAT_DIFFUSE = 0,         /* Diffuse(Kd)                           Diffuse.cpp:17-20  */
    ORX_MAT_DIFFUSE_EMITTER = 1, /* DiffuseEmitter(power, Kd)+inverseArea DiffuseEmitter.cpp:17-25 */
    ORX_MAT_MIRROR = 2,          /* Mirror(Kr)                            Mirror.cpp:17-20   */
    ORX_MAT_GLASS = 3,           /* Glass(ior, Kr, Kt)                    Glass.cpp:17-22    */
    ORX_MAT_GLOSSY = 4,          /* Glossy(Kd, Ks, exponent)              Glossy.cpp:16-33   */
    ORX_MAT_TEXTURE = 5          /* Texture(diffuse map [, normal map])   Texture.cpp:18-29  */
} orx_material_type;

typedef struct {
    int32_t type;        /* orx_material_type */
    float Kd[3];         /* diffuse albedo (Diffuse, Glossy, DiffuseEmitter) */
    float Ks[3];         /* Glossy specular */
    float Kr[3];         /* Mirror / Glass reflectance */
    float Kt[3];         /* Glass transmittance */
    float ior;           /* Glass index of refraction */
    float exponent;      /* Glossy Phong exponent */
    float power[3];      /* DiffuseEmitter power (scaled by Kd inside the engine, as the ctor does) */
    float inverse_area;  /* DiffuseEmitter 1/area of the emitting quad */
    int32_t texture;     /* Texture: index into orx_scene.textures */
} orx_material;

/* Texture images (util/Image.cpp): RGBA8 rows, row 0 first, sampled as
 * rtTextureSampler<uchar4, 2, cudaReadModeNormalizedFloat> with bilinear
 * filtering, wrap addressing and normalised coordinates (Texture.cpp:109-122). */
typedef struct {
    uint32_t width, height;
    const uint8_t* rgba;          /* width * height * 4: diffuseSampler */
    uint32_t normal_width, normal_height;
    const uint8_t* normal_rgba;   /* normalMapSampler, or NULL (hasNormals = 0) */
} orx_texture;

/* Light::LightType (renderer/Light.h:14-54). */
typedef enum { ORX_LIGHT_AREA = 0, ORX_LIGHT_POINT = 1, ORX_LIGHT_SPOT = 2 } orx_light_type;

typedef struct {
    int32_t type;        /* orx_light_type */
    float power[3];
    float position[3];   /* area: anchor */
    float v1[3];         /* area: edge 1 */
    float v2[3];         /* area: edge 2 */
    float direction[3];  /* spot */
    float angle;         /* spot, degrees */
} orx_light;

/* Flattened scene (replaces IScene::getSceneRootGroup's OptiX node graph).
 * Deep-copied by orx_init_scene.  Primitive order defines the tie-break of
 * equal-distance hits (lowest global primitive id wins): quads first, then
 * spheres, then triangles. */
typedef struct {
    uint32_t n_quads;
    const float* quads;              /* n_quads * 9: anchor, offset1, offset2 (Cornell.cpp:33-64) */
    const uint32_t* quad_material;   /* n_quads */
    uint32_t n_spheres;
    const float* spheres;            /* n_spheres * 4: center xyz, radius (Sphere.cu) */
    const uint32_t* sphere_material; /* n_spheres */
    uint32_t n_vertices;
    const float* vertices;           /* n_vertices * 3 */
    const float* normals;            /* n_vertices * 3 or NULL (TriangleMesh.cu:56-59) */
    uint32_t n_triangles;
    const uint32_t* triangles;       /* n_triangles * 3 vertex indices */
    const uint32_t* triangle_material;
    uint32_t n_materials;
    const orx_material* materials;
    uint32_t n_lights;
    const orx_light* lights;         /* IScene::getSceneLights */
    float aabb_min[3];               /* IScene::getSceneAABB */
    float aabb_max[3];
    /* TriangleMesh.cu attribute buffers (Scene.cpp:395-440) */
    const float* texcoords;          /* n_vertices * 2 or NULL (textureCoordinate = 0) */
    const float* tangents;           /* n_vertices * 3 or NULL; with bitangents: hasTangentsAndBitangents */
    const float* bitangents;         /* n_vertices * 3 or NULL */
    uint32_t n_textures;
    const orx_texture* textures;
    /* participating media (AABInstance + ParticipatingMedium(sigma_s, sigma_a), Scene.cpp:337-350):
     * at most one axis-aligned box; used when orx_config.enable_media is set */
    uint32_t n_media;
    const float* media;              /* n_media * 8: box min xyz, box max xyz, sigma_s, sigma_a */
} orx_scene;

/* Compile-time constants of config.h / OptixRenderer.cpp:38-61 as runtime config. */
typedef struct {
    uint32_t photon_launch_width;     /* PHOTON_LAUNCH_WIDTH  = 1024 */
    uint32_t photon_launch_height;    /* PHOTON_LAUNCH_HEIGHT = 1024 */
    uint32_t max_photon_deposits;     /* MAX_PHOTONS_DEPOSITS_PER_EMITTED = 4 */
    uint32_t photon_grid_max_size;    /* PHOTON_GRID_MAX_SIZE = 100*100*100 */
    uint32_t max_photon_trace_depth;  /* MAX_PHOTON_TRACE_DEPTH = 7 */
    uint32_t max_radiance_trace_depth;/* MAX_RADIANCE_TRACE_DEPTH = 9 */
    uint32_t vcm_max_path_length;     /* VCM_MAX_PATH_LENGTH = 10 */
    uint32_t seed;                    /* 0: 574133*clock()+47844152748*time() like SpatialHash.cu:322; else DEBUG_RANDOM_SEED */
    uint32_t debug_counters;          /* 1: keep per-pixel cells/photons visited (OptixRenderer.cpp:872-953) */
    uint32_t gather_variant;          /* photon-grid layout for the gather: 2 photons ordered by cell-row
                                         quarter sub-rows (y and z halves) and x quarters; 1 photons in cell
                                         order with x quarters only; 0 (default) the faster of the two for the
                                         renderer: sub-rows on a single device, cell order for a shard of
                                         world >= 2 (orx_set_shard: it holds 1/N of the photons, so the
                                         per-sub-row work outweighs the photons it trims).  The image does not
                                         depend on it.  Any other value: ORX_ERR_INVALID_ARGUMENT */
    uint32_t photon_map;              /* ACCELERATION_STRUCTURE (config.h): 0 uniform grid (the shipped
                                         configuration), 1 stochastic hash (OptixRenderer_SpatialHash.cu:286-302,
                                         store_photon.h, IndirectRadianceEstimation.cu:131-162; needs
                                         PW*PH*max deposits a power of two, one rank, trace depth <= 9),
                                         2 kd-tree (ACCELERATION_STRUCTURE_KD_TREE_CPU:
                                         OptixRenderer_CPUKdTree.cpp, IndirectRadianceEstimation.cu:164-209;
                                         built on the device here) */
    uint32_t enable_media;            /* ENABLE_PARTICIPATING_MEDIA (config.h:29): the scene's medium box
                                         (orx_scene.media) scatters photons and eye rays gather its volumetric
                                         photons (ParticipatingMedium.cu, VolumetricPhotonSphere*.cu); the PPM
                                         direct pass takes no shadow samples (DirectRadianceEstimation.cu:54).
                                         All of this applies only when the scene has a medium box: with
                                         enable_media set and orx_scene.n_media == 0 the renderer runs exactly
                                         as with enable_media = 0 (the direct pass keeps its 4 shadow samples,
                                         unlike a reference build with the macro on).  PPM on one device only
                                         (other methods / world > 1: ORX_ERR_UNSUPPORTED) */
    uint32_t volumetric_photons;      /* NUM_VOLUMETRIC_PHOTONS = 200000 (config.h:35): volumetric photon table */
    uint32_t vcm_merging;             /* m_vcmUseVM (OptixRenderer.cpp:301): 0 (default, the reference's shipped
                                         configuration) VCM is vertex connection only; 1 adds vertex merging: every
                                         non-specular camera vertex gathers the light vertices of ALL subpaths
                                         within ppm_radius (Georgiev et al., VCM tech. rep. eqs. 37-41; SmallVCM
                                         RangeQuery::Process), and every connection weight takes misVm = etaVCM
                                         (orx_vcm_mis_factors).  There is no combined path-length cap: the fork's
                                         connectVertices has none either (vcm.h:315-400), so connection and merging
                                         weight the same path set.  A merging iteration runs its passes serially
                                         (light pass, light-vertex grid, walk, resolve, merge, sum: orx_ppm_pipelined
                                         returns 0) on one device: orx_vcm_local_light with world > 1 gives
                                         ORX_ERR_UNSUPPORTED (a rank would need every rank's light vertices).  PT and
                                         PPM requests are unaffected.  The camera-vertex cache takes
                                         vcm_max_path_length * W * rows * 64 B (1.33 GB at 1080p), allocated by the
                                         first VCM iteration.  Any other value: ORX_ERR_INVALID_ARGUMENT */
    uint32_t reserved[2];
} orx_config;

void orx_default_config(orx_config* cfg);
/* The VCM MIS constants of one iteration (OptixRenderer.cpp:677-696 in float; pure, host only: no
 * renderer and no device), as every VCM iteration computes them:
 *   etaVCM = (float)(width * height) * pi * radius^2      (nVM / nVC = lightSubpathCount, evaluated left to right)
 *   *mis_vc = 1 / etaVCM
 *   *mis_vm = merging ? etaVCM : 0
 *   *vm_normalization = 1 / (radius^2 * pi * (float)(width * height))
 * A NULL output: ORX_ERR_INVALID_ARGUMENT. */
orx_status orx_vcm_mis_factors(uint32_t width, uint32_t height, float radius, int merging, float* mis_vc,
                               float* mis_vm, float* vm_normalization);

orx_status orx_create(int hip_device, const orx_config* cfg, orx_renderer** out);
orx_status orx_init_scene(orx_renderer* r, const orx_scene* scene);
orx_status orx_render_next_iteration(orx_renderer* r, uint64_t iteration_number,
                                     uint64_t local_iteration_number, float ppm_radius,
                                     int create_output, const orx_request* details);
/* W*H*3 floats into caller-owned host memory; SUM over local iterations. */
orx_status orx_get_output(orx_renderer* r, float* dst, size_t dst_bytes);
/* Same, device-to-device into caller-owned device memory on the renderer's
 * device (used by the multi-GPU harness to hand the buffer to RCCL). */
orx_status orx_get_output_device(orx_renderer* r, void* dst_device, size_t dst_bytes);
uint32_t orx_width(const orx_renderer* r);
uint32_t orx_height(const orx_renderer* r);
size_t orx_output_bytes(const orx_renderer* r);
uint32_t orx_emitted_photons_per_iteration(const orx_renderer* r);
const char* orx_last_error(const orx_renderer* r);
void orx_destroy(orx_renderer* r);

/* ---- inspection (parity tests, profiling; not part of the reference API) ---- */
/* test hook: pretend the photon pass's deep-stack buffer covers only `lanes` lanes (bookkeeping only;
 * the next resize or initScene sizes it again), so that the next PPM photon pass must return
 * ORX_ERR_STATE instead of launching past the buffer (OptixRenderer.cpp:816-820 throws) */
orx_status orx_debug_limit_photon_stack(orx_renderer* r, uint32_t lanes);
/* test hook: rerun the last VCM iteration's resolve (deferred shadow rays, colours) with stale list
 * state -- entry count past the capacity, odd pixels' list heads past the entries, light-connection
 * entries whose pixel offsets lie past the light image -- which the resolve's device-side bounds must
 * absorb; synchronous, colours in ORX_BUF_VCM_CAMERA (the output is accumulated once more) */
orx_status orx_debug_vcm_stale_resolve(orx_renderer* r);
typedef enum {
    ORX_BUF_RNG = 0,        /* uint32 [slots][6]: xorwow v0..v4, d */
    ORX_BUF_HITPOINTS = 1,  /* float  [W*H][13]: pos3 normal3 atten3 radiance3 flags(bits) */
    ORX_BUF_PHOTONS = 2,    /* float  [S][9] grid-sorted photons: power3 position3 direction3 (valid prefix);
                               stochastic hash: [photonsSize][9] the photon each table entry holds (0 if empty) */
    ORX_BUF_GRID_OFFSETS = 3,/* uint32 [G+1]; stochastic hash: [photonsSize] photonsHashTableCount */
    ORX_BUF_INDIRECT = 4,   /* float  [W*H][3] */
    ORX_BUF_DIRECT = 5,     /* float  [W*H][3] */
    ORX_BUF_OUTPUT = 6,     /* float  [W*H][3] */
    ORX_BUF_PHOTON_SLOTS = 7,/* float [S][9] unsorted photon slots: power3 position3 direction3 (0 when cleared) */
    ORX_BUF_DEBUG_VISITED = 8,/* uint32 [W*H][2]: cells visited, photons visited */
    /* VCM (vcm/VCMLightPass.cu, VCMCameraPass.cu); light subpath p = x + y*W pairs with pixel p */
    ORX_BUF_VCM_VERTEX_COUNT = 9, /* uint32 [W*H]: stored light vertices per subpath (lightSubpathVertexCountBuffer) */
    ORX_BUF_VCM_VERTICES = 10,    /* float [9][W*H][16]: per vertex slot k, subpath p: pos3 mat(bits) throughput3 dVCM
                                     normal3 dVC dirFix3 dVM; entries k >= count[p] are stale */
    ORX_BUF_VCM_SPLAT = 11,       /* float [W*H][3]: this iteration's light-tracing splats (connectCameraT1) */
    ORX_BUF_VCM_CAMERA = 12,      /* float [W*H][3]: this iteration's camera subpath colour (cameraPrd.color) */
    /* kd-tree photon map (photon_map = 2): the implicit tree m_photonKdTree of pow2roundup(S + 1) - 1 nodes,
       node i's children at 2i+1, 2i+2; per node power3 position3 direction3 axis(uint32 bits: PPM_X 1, PPM_Y 2,
       PPM_Z 4, PPM_LEAF 8, PPM_NULL 16, config.h:12-16).  Only nodes reachable from the root are defined (the
       reference never clears the buffer; a NULL node defines axis and power only). */
    ORX_BUF_KD_TREE = 13,
    /* participating medium (orx_config.enable_media) */
    ORX_BUF_VOLUMETRIC = 14,        /* float [W*H][3]: the last eye pass's Hitpoint::volumetricRadiance */
    ORX_BUF_VOLUMETRIC_PHOTONS = 15,/* float [volumetric_photons][7]: the last photon pass's volumetric photon
                                       table, power3 position3 numDeposits(uint32 bits); 0 when empty */
    /* vertex merging (orx_config.vcm_merging = 1; ORX_ERR_STATE with merging off or before a VCM iteration) */
    ORX_BUF_VCM_CAMERA_VERTEX_COUNT = 16, /* uint32 [W*H]: merging vertices stored per camera subpath */
    ORX_BUF_VCM_CAMERA_VERTICES = 17,     /* float [vcm_max_path_length][W*H][16]: per record slot k, pixel p, the
                                     k-th camera vertex at which connections are made: pos3 mat(bits) throughput3 dVCM
                                     normal3 dVM direction3 0: the hit point and its material id, the subpath
                                     throughput and dVCM, the geometric normal and dVM (both MIS terms after
                                     mis_on_hit at the vertex, before scattering) and the world direction of the
                                     ray that arrived; entries k >= count[p] are stale.  The texel colour of a
                                     Texture vertex does not fit the 64-B record: it is kept in a plane beside it,
                                     as for the light vertices, and is not part of this buffer */
    ORX_BUF_VCM_MERGE = 18,         /* float [W*H][3]: this iteration's merging colour (times throughput and
                                       normalisation); ORX_BUF_VCM_CAMERA then holds connections + merging */
    ORX_BUF_VCM_MERGE_COUNT = 19,   /* uint32 [W*H]: accepted (camera vertex, light vertex) pairs (d2 <= r2) of the
                                       pixel; only with debug_counters = 1 (ORX_ERR_STATE otherwise) */
    ORX_BUF_VCM_MERGE_CANDIDATES = 20,/* uint32 [W*H]: the pairs whose distance the pixel's range queries tested;
                                       only with debug_counters = 1 */
    /* convergence statistics (orx_set_convergence; ORX_ERR_STATE while they are off), over the renderer's own rows */
    ORX_BUF_CONV_PREV = 21,  /* float [rows*W][3]: the running sum after the last iteration */
    ORX_BUF_CONV_SUM = 22,   /* float [rows*W]: A, the window's sum of per-iteration luminances */
    ORX_BUF_CONV_M2 = 23,    /* float [rows*W]: M2, the Welford sum of squared deviations */
    ORX_BUF_CONV_ERROR = 24  /* float [rows*W]: the error plane of the last orx_get_convergence (ORX_ERR_STATE
                                before one) */
} orx_buffer_id;
/* Copies buffer `id` to host; returns the byte size through *out_bytes
 * (call with dst=NULL to query). */
orx_status orx_read_buffer(orx_renderer* r, int32_t id, void* dst, size_t dst_bytes, size_t* out_bytes);

/* Passes timed with HIP events on the renderer's stream. */
typedef enum {
    ORX_PASS_PPM_EYE = 0,      /* PPM_RAYTRACE_PASS */
    ORX_PASS_PPM_PHOTON = 1,   /* PPM_PHOTON_PASS (+ fused photon AABB) */
    ORX_PASS_GRID_HASH = 2,    /* grid setup + calculateHashCellsKernel + histogram */
    ORX_PASS_GRID_SCAN = 3,    /* exclusive scan -> hashmapOffsetTable */
    ORX_PASS_GRID_SCATTER = 4, /* sort_by_key as counting-sort scatter */
    ORX_PASS_PPM_GATHER = 5,   /* PPM_INDIRECT_RADIANCE_ESTIMATION_PASS */
    ORX_PASS_PPM_DIRECT = 6,   /* PPM_DIRECT_RADIANCE_ESTIMATION_PASS + PPM_OUTPUT_PASS */
    ORX_PASS_PT = 7,           /* PT_RAYTRACE_PASS */
    ORX_PASS_VCM_LIGHT = 8,    /* VCM_LIGHT_PASS */
    ORX_PASS_VCM_CAMERA = 9,   /* VCM_CAMERA_PASS: the camera subpaths and their connections */
    ORX_PASS_VCM_SHADOW = 10,  /* VCM_CAMERA_PASS, second half: the connections' deferred shadow rays and colours */
    ORX_PASS_VCM_GRID = 11,    /* vertex merging: the light-vertex grid (keys, sort, cell starts, records) */
    ORX_PASS_VCM_MERGE = 12,   /* vertex merging: the camera vertices' range queries and the per-pixel sum */
    ORX_PASS_CONVERGENCE = 13, /* the per-pixel statistics update behind an iteration's last write to the running sum
                                  (orx_set_convergence; nothing is launched or timed while it is off) */
    ORX_PASS_COUNT = 14
} orx_pass;

typedef struct {
    uint32_t grid_size[3];
    float cell_size;
    float world_origin[3];
    uint32_t valid_photons;      /* photons in the grid (offset[G]) of the last iteration */
    uint32_t num_cells;
    uint64_t photons_visited;    /* gather: photons visited, last iteration (debug counters) */
    uint64_t cells_visited;      /* gather: (y,z) cell rows visited, last iteration */
    uint64_t photons_visited_total; /* summed since orx_reset_timing */
    uint64_t cells_visited_total;
    uint64_t valid_photons_total;
    uint32_t vcm_shadow_rays;     /* VCM: connection shadow rays the last camera pass deferred (launch_vcm_camera) */
    uint32_t vcm_shadow_overflow; /* VCM: 1 if they exceeded the entry list and the pass reran in place */
    uint32_t timed_iterations;   /* iterations since orx_reset_timing */
    uint32_t bvh_stack_entries;  /* LDS traversal stack depth bound of the scene's BVH4 */
    float pass_ms[16];           /* device time per orx_pass summed since orx_reset_timing */
    uint32_t vcm_light_connections; /* VCM: the last light pass's camera connections deferred to the resolve */
    uint32_t vcm_light_inplace;     /* VCM: of its connections, those traced in the light pass (list full) */
} orx_stats;
orx_status orx_get_stats(orx_renderer* r, orx_stats* out);
/* starts a new timed region for orx_get_stats' *_total and pass_ms fields */
orx_status orx_reset_timing(orx_renderer* r);
/* 1 if the last iteration ran pipelined: PPM, its gather and output pass (ORX_PASS_PPM_GATHER and the
 * output half of ORX_PASS_PPM_DIRECT) on a second stream beside the next iteration's eye, photon and
 * grid passes; VCM, its deferred shadow rays and colours (ORX_PASS_VCM_SHADOW) beside the next
 * iteration's light pass and camera subpaths; so those pass_ms are overlapped wall time; 0 otherwise */
int orx_ppm_pipelined(const orx_renderer* r);
/* The single-device pipelined PPM schedule's grid build (uniform grid): 0 on the renderer's stream before
 * the next photon pass, 1 on a stream of its own beside it, -1 not chosen yet.  By default (ORX_GRID_ASYNC
 * unset) the renderer chooses after the first pipelined iterations following a resize: the first is timed
 * (its photon pass + grid build, and its gather, which the next photon pass then waits for), and the
 * asynchronous build is taken when photon + grid exceed 1.15x the gather; ORX_GRID_ASYNC=0 / 1 fixes it.
 * probe_ms (optional, 2 floats): the measured photon + grid and gather times (ms; 0 when not measured).
 * No reference counterpart (OptiX schedules its own launches); images are identical either way. */
int orx_ppm_grid_schedule(const orx_renderer* r, float* probe_ms);
/* Single-device PPM iteration pipelining and VCM shadow-ray overlap: 1 on, 0 off (serial passes), -1
 * the ORX_PIPELINE environment default (on).  Takes effect at the next iteration (an outstanding pipelined
 * iteration is finished first); images are identical either way. */
orx_status orx_set_iteration_pipelining(orx_renderer* r, int mode);

/* ---- Convergence estimate and 8-bit display resolve ----
 * Two passes over the running sum, after an iteration's last write to it; no render kernel changes and the
 * reference has no counterpart for the first (its hosts render a fixed number of iterations).
 *
 * orx_set_convergence: per-pixel statistics of the iterations' luminances, off by default.  Off launches and
 * allocates nothing.  On, the renderer keeps 20 B per own pixel: prev[3] (the running sum after the previous
 * iteration), A (sum of the window's per-iteration luminances) and M2 (Welford's sum of squared deviations),
 * updated on the stream, and at the point, where the iteration's last write to the running sum S is enqueued
 * (the pipelined gather stream, the overlapped VCM resolve's stream, a sharded renderer's finish), in fp32 and
 * in this order, n being the iteration's number within the window:
 *     d = S - prev  per channel (prev taken as 0 when the iteration is the window's first and cleared the sum)
 *     y = (0.2126f d.r + 0.7152f d.g) + 0.0722f d.b
 *     n == 1: A = y, M2 = 0
 *     n >= 2: mo = A / (float)(n - 1), A = A + y, mn = A / (float)n, M2 = M2 + (y - mo) (y - mn)
 *     prev = S
 * The iteration's radiance is taken as a difference of running sums, which costs one rounding of S per
 * iteration (relative to one iteration's value about n * 6e-8); in return every kernel that writes the sum
 * stays as it is.  A new window starts when the statistics are switched on (again), at a resize, at an
 * iteration with local_iteration_number 0 and at a restore of a checkpoint; switched on mid-render, or after a
 * restore, the current sum is the window's base and the window counts from the next iteration.  The
 * statistics are not part of a checkpoint.
 *
 * orx_get_convergence (synchronous, as orx_get_output; it finishes what is outstanding first): per pixel
 *     se = sqrtf(M2 / ((float)n (float)(n - 1))),  m = A / (float)n,  e = se / fmaxf(m, floor)
 * the relative standard error of the pixel's mean luminance, reduced on the device per 16x16 tile of global
 * pixel coordinates (partial tiles average over the pixels that exist); the frame means are finished on the
 * host in double.  tile_error (optional) receives the tile means, [tiles_y][tiles_x].  A pixel whose iterations
 * are equal up to rounding can leave M2 a few ulp^2 below zero; its e is then NaN, it counts as not above the
 * threshold and its tile is never the worst, but the frame and tile means that include it are NaN, which no
 * comparison "<= E" accepts.  ORX_ERR_STATE: statistics
 * off, fewer than 2 iterations in the window, or a sharded renderer of world > 1 (its group answers);
 * ORX_ERR_INVALID_ARGUMENT: floor not finite and > 0, threshold NaN, out NULL, tile_bytes too small. */
typedef struct {
    uint32_t iterations;        /* n of the window */
    uint32_t tiles_x, tiles_y;  /* ceil(W/16), ceil(H/16) */
    uint32_t pixels_above;      /* pixels with error > threshold */
    uint32_t max_tile;          /* tx + tiles_x*ty of the worst tile */
    float mean_error;           /* mean over pixels */
    float max_tile_error;       /* largest tile mean */
    float mean_luminance;       /* mean over pixels of A/n */
    uint32_t reserved[3];
} orx_convergence;
orx_status orx_set_convergence(orx_renderer* r, int enable);
orx_status orx_get_convergence(orx_renderer* r, float floor, float threshold, orx_convergence* out,
                               float* tile_error /* [tiles_y][tiles_x] or NULL */, size_t tile_bytes);

/* The display rule of the reference's consumer (Gui/gui/RenderWidget.cpp:197, :296-313), per channel c of the
 * running sum, with the deterministic power function of orx_detmath.h (include/orx_display.h holds the one
 * function the host call and the kernel share):
 *     v = c * inv_iterations;  !(v > 0) (zero, negative, NaN): byte 0
 *     else g = pow(v, inv_gamma) * 255.f, byte = (uint8_t)fminf(255.f, g)  (truncation; inf gives 255)
 * and alpha 255; 4 bytes per pixel, R G B A or B G R A in memory.  orx_display_convert is pure host code
 * (no device); orx_get_display resolves the renderer's own rows on the device into a renderer-owned image and
 * copies rows*W*4 bytes (synchronous; works with the statistics off); both give the same bytes.
 * ORX_ERR_STATE before the first frame; ORX_ERR_INVALID_ARGUMENT: a factor not finite and > 0, an unknown
 * format, a NULL pointer, dst_bytes too small. */
typedef enum { ORX_DISPLAY_RGBA8 = 0, ORX_DISPLAY_BGRA8 = 1 } orx_display_format;
orx_status orx_display_convert(const float* sum, size_t n_pixels, float inv_iterations, float inv_gamma,
                               int32_t format, uint8_t* dst);
orx_status orx_get_display(orx_renderer* r, float inv_iterations, float inv_gamma, int32_t format,
                           uint8_t* dst, size_t dst_bytes);

/* ---- Multi-GPU sharding ----
 * Rank `rank` of `world` owns every RNG-slot row y with y % world == rank:
 * its pixel rows and its photon-launch rows (photon thread (x,y) aliases RNG
 * slot (x,y), OptixRenderer_SpatialHash.cu:310-334), so RNG states never
 * leave their GPU.  cfg.photon_launch_height is the GLOBAL launch height.
 * One PPM iteration of a sharded renderer is driven by the caller:
 *   orx_ppm_local_passes      eye pass (own pixel rows), photon pass (own rows), photon grid (own photons)
 *   orx_export_hitpoints      own hitpoints -> caller buffer (orx_hitpoint_export_bytes)
 *   (caller all-gathers the export buffers of all ranks, rank-major)
 *   orx_ppm_gather_external   gather every rank's hitpoints against the own grid -> partial indirect
 *   (caller reduce-scatters (sum) the partial indirect buffers, rank-major blocks)
 *   orx_ppm_finish            direct pass + output accumulation on own rows
 * The sum over ranks of the partial gathers equals the single-GPU gather up
 * to fp32 summation order (the gather is linear in the photon set and its
 * normalisation uses the global emitted count).  orx_render_next_iteration
 * is the world == 1 composition of the same phases.  With world > 1,
 * orx_get_output returns only the rank's own rows (local row j = global
 * row rank + j*world). */
orx_status orx_set_shard(orx_renderer* r, uint32_t rank, uint32_t world);
/* hipStream_t the renderer launches on (as void*). */
void* orx_stream(orx_renderer* r);
/* use_external != 0: launch everything on the caller's hipStream_t `hip_stream`
 * (NULL = the legacy default stream), e.g. torch's current stream, so kernels
 * and the caller's collectives are ordered; use_external == 0: own stream. */
orx_status orx_set_stream(orx_renderer* r, void* hip_stream, int use_external);
/* rows owned by this rank for the current resolution, and ceil(H/world) */
uint32_t orx_local_rows(const orx_renderer* r);
uint32_t orx_max_local_rows(const orx_renderer* r);
/* P * 28 with P = max_local_rows * W rounded up to a multiple of 4: plane A (position | flags bits,
 * float4) then plane N (the normal of a non-specular hit, the radiance of another, float3), P
 * pixels each (the padding keeps every segment of an all-gathered buffer 16-B aligned).  The
 * attenuation stays with the owner: orx_ppm_gather_external returns the unattenuated estimate
 * (sum of weighted photon powers / (pi r^2 emitted)) and orx_ppm_finish multiplies the summed own
 * rows by their hit points' attenuation (IndirectRadianceEstimation.cu:220; fp32 order differs) */
size_t orx_hitpoint_export_bytes(const orx_renderer* r);
orx_status orx_ppm_local_passes(orx_renderer* r, uint64_t iteration_number, uint64_t local_iteration_number,
                                float ppm_radius, const orx_request* details);
/* the two halves of orx_ppm_local_passes, so that the hitpoint all-gather can
 * overlap the photon pass: eye pass only / photon pass + grid only */
orx_status orx_ppm_local_eye(orx_renderer* r, uint64_t iteration_number, uint64_t local_iteration_number,
                             float ppm_radius, const orx_request* details);
orx_status orx_ppm_local_photons(orx_renderer* r);
orx_status orx_export_hitpoints(orx_renderer* r, void* dst_device, size_t dst_bytes);
/* hitpoints_device: `segments` export buffers back to back; indirect_device:
 * segments * max_local_rows * W * 3 floats */
orx_status orx_ppm_gather_external(orx_renderer* r, const void* hitpoints_device, uint32_t segments,
                                   void* indirect_device, size_t indirect_bytes);
/* indirect_device: max_local_rows * W * 3 floats for the own rows: the summed unattenuated
 * estimates (times each own hit point's attenuation here) */
orx_status orx_ppm_finish(orx_renderer* r, const void* indirect_device, size_t indirect_bytes);
/* orx_ppm_finish on `stream` (a hipStream_t; NULL: as orx_ppm_finish).  Pipelined (orx_set_ppm_pipeline), the
 * finish of iteration i may be issued after iteration i+1's orx_ppm_local_eye -- behind i+1's hit-point
 * all-gather, so that the reduce-scatter of i does not hold that all-gather back on RCCL's in-order stream --
 * and then finishes i (its pixel buffers and constants are held for it); at most one such finish may be
 * outstanding when the next eye pass is issued (ORX_ERR_STATE otherwise) */
orx_status orx_ppm_finish_on(orx_renderer* r, const void* indirect_device, size_t indirect_bytes, void* stream);
/* Pipelined sharded PPM (uniform grid or kd-tree: the hash is single-device, and pipelines on
 * its own without this call; call before the first iteration, like orx_set_shard):
 * orx_ppm_gather_external and orx_ppm_finish of iteration i run on `side_stream` (a hipStream_t
 * of the caller's, who also issues the indirect reduce-scatter there), overlapping iteration
 * i+1's eye, photon and grid passes on the renderer's stream; the direct pass runs on an internal
 * stream right after the photon pass.  Two buffer sets alternate, events order the RNG chain and
 * buffer reuse; the caller makes `side_stream` wait for the hitpoint all-gather before the
 * gather.  enable = 0 restores the serial phases. */
orx_status orx_set_ppm_pipeline(orx_renderer* r, void* side_stream, int enable);

/* Spatial photon partition of the sharded gather ("slab mode", uniform grid only; call before the
 * first iteration, like orx_set_shard).  Rank g owns a slab of bins of one axis of the scene AABB:
 * it receives the photons of ALL ranks in its slab plus those within halo_bins bins of it, and
 * gathers exactly the non-specular hit points whose position lies in its slab, so every hit point
 * is gathered once, with its complete window, and the gather's per-pixel work divides by N (the
 * row partition above gathers all W*H hit points on every rank).  One PPM iteration:
 *   orx_ppm_local_eye + orx_ppm_local_photon_trace   (or orx_ppm_local_trace: both)  eye pass,
 *                            photon pass of the own rows; no grid yet
 *   orx_ppm_slab_histogram   per-bin counts [2][3][nbins] (uint32): the own valid deposits and the
 *                            own non-specular hit points, per axis, nbins bins over the scene AABB
 *                            (nbins a multiple of ORX_SLAB_VOXELS, at most 1024); then 6 words: the
 *                            AABB of the own deposits as order-preserving integers (f >= 0:
 *                            bits | 2^31, f < 0: ~bits; empty: lo 0xffffffff, hi 0); then
 *                            [2][V^3] counts of both over V = ORX_SLAB_VOXELS voxels per axis of
 *                            the scene AABB (x + V (y + V z)): orx_slab_histogram_words(nbins) words
 *   (caller all-gathers the histograms and plans on the host, e.g. with orx_slab_plan below: one axis
 *    and a bin -> rank table, the same on every rank; photons from rank s to rank d = the sum of s's
 *    photon bins mapped to d)
 *   orx_ppm_slab_pack        the own valid deposits, rank-major into the caller's send buffer: a
 *                            photon in bin b goes to every rank from bin_dest[b - halo_bins] to
 *                            bin_dest[b + halo_bins] (clamped; bin_dest ascending), at dest_base[d] + k
 *                            for the k-th photon sent to d (9 floats each: position, direction,
 *                            power); host arrays bin_dest[nbins], dest_base[world].  halo_bins >=
 *                            floor(r / bin width) + 2 makes every photon within r of a hit point
 *                            reach the hit point's owner
 *   (caller all-to-alls the photon records)
 *   orx_ppm_slab_import      the received records become this rank's photon set; grid build over
 *                            photon_box (host, 6 words as above: the min/max over ranks of the
 *                            histograms' AABBs, so every rank's grid has the single-device grid's
 *                            origin and cell size; NULL: the AABB of the imported photons); the
 *                            rank owns the hit points whose bin on `axis` lies in [own_lo, own_hi]
 *                            (own_lo > own_hi: none)
 *   orx_export_hitpoints / orx_ppm_gather_external / orx_ppm_finish as above (the gather skips hit
 *   points whose sphere misses this rank's photon grid)
 * Each hit point's indirect comes whole from its owner (the others write 0), so the reduce-scatter
 * sum is the single-GPU gather of that pixel up to fp32 order inside its window.  Capacity: the
 * import takes up to the global photon launch's deposit slots (PW * PH * max deposits) per rank. */
#define ORX_SLAB_VOXELS 32u
/* 6 nbins + 6 + 2 ORX_SLAB_VOXELS^3 */
size_t orx_slab_histogram_words(uint32_t nbins);
orx_status orx_set_slab_partition(orx_renderer* r, int enable);
orx_status orx_ppm_local_trace(orx_renderer* r, uint64_t iteration_number, uint64_t local_iteration_number,
                               float ppm_radius, const orx_request* details);
orx_status orx_ppm_local_photon_trace(orx_renderer* r);
orx_status orx_ppm_slab_histogram(orx_renderer* r, uint32_t* hist_device /* orx_slab_histogram_words */,
                                  uint32_t nbins);
/* the halo for radius r: floor(r * nbins / extent of the scene AABB on axis) + 2 bins */
uint32_t orx_ppm_slab_halo(const orx_renderer* r, uint32_t nbins, uint32_t axis, float radius);
orx_status orx_ppm_slab_pack(orx_renderer* r, const uint8_t* bin_dest, uint32_t nbins, uint32_t axis,
                             uint32_t halo_bins, const uint32_t* dest_base, uint64_t send_records,
                             void* send_device);
orx_status orx_ppm_slab_import(orx_renderer* r, const void* recv_device, uint64_t n_records,
                               const uint32_t* photon_box, uint32_t axis, uint32_t nbins, uint32_t own_lo,
                               uint32_t own_hi);

/* One VCM iteration of a sharded renderer (OptixRenderer.cpp:675-795 split at
 * the light-tracing splats).  Light subpath i pairs with camera pixel i
 * (lightSubpathCount = W*H, VCMLightPass.cu:52), so each rank traces the light
 * subpaths and camera paths of its own rows; the only cross-rank effect is
 * connectCameraT1 (vcm.h:311-384), whose splats may land on any row:
 *   orx_vcm_local_light     light pass over own rows; splats into an owner-block
 *                           buffer [world][max_local_rows][W][3]
 *   orx_export_vcm_splats   that buffer -> caller (orx_vcm_splat_bytes)
 *   (caller reduce-scatters (sum) the buffers, rank-major blocks)
 *   orx_vcm_finish          camera pass over own rows with the summed own-row splats
 * The summed splats equal the single-GPU ones up to fp32 atomic order (the
 * single-GPU pass accumulates them with atomics too). */
size_t orx_vcm_splat_bytes(const orx_renderer* r); /* world * max_local_rows * W * 12 */
orx_status orx_vcm_local_light(orx_renderer* r, uint64_t iteration_number, uint64_t local_iteration_number,
                               float ppm_radius, const orx_request* details);
orx_status orx_export_vcm_splats(orx_renderer* r, void* dst_device, size_t dst_bytes);
/* splat_own_rows_device: local_rows * W * 3 floats (the own block of the sum) */
orx_status orx_vcm_finish(orx_renderer* r, const void* splat_own_rows_device, size_t bytes);

/* ---- Multi-GPU render groups ----
 * N renderers ("ranks") and the collectives between them behind one handle, so that a C++ host drives
 * an N-GPU frame with the call sequence of one renderer and no collective of its own: the phases above
 * (ROWS) or whole iterations (BATCH) are scheduled inside.  The reference's counterparts:
 * DistributedApplication.cpp:96-122 deals iteration numbers and radii to the render servers,
 * RenderServerRenderer.cpp:146-165 renders each request, RenderResultPacketReceiver.cpp:63-190 merges the
 * running sums.
 *
 * ORX_GROUP_ROWS   one call renders one frame over the ranks: rank k is a renderer on hip_devices[k] with
 *                  the shard (k, n) of the row partition above; cfg.photon_launch_height is the global launch
 *                  height.  PPM, pipeline = 1: eye pass and export; hit-point all-gather; the previous
 *                  iteration's reduce-scatter and finish on a finish stream, issued behind that all-gather;
 *                  photon pass and grid; gather on a side stream: two buffer sets, no host synchronisation
 *                  in steady state.  pipeline = 0: the serial phases.  VCM reduce-scatters the splats, PT
 *                  needs no exchange.  The schedule keeps seven streams per rank busy: with fewer than 8
 *                  hardware queues (GPU_MAX_HW_QUEUES) they share queues and partly serialise.  The
 *                  stochastic hash (photon_map = 1) and participating media are single-device: n > 1 gives
 *                  ORX_ERR_UNSUPPORTED.
 *                  photon_partition = ORX_PHOTONS_ROWS (default): every rank gathers all W*H hit points
 *                  against the photons of its own launch rows.  ORX_PHOTONS_SLABS: the spatial photon
 *                  partition above (orx_set_slab_partition) for PPM frames, planned and exchanged inside
 *                  the group: after the photon pass each rank's histogram is all-gathered and copied to the
 *                  host (from rank 0), orx_slab_plan chooses the axis and the bin -> rank table, the ranks
 *                  pack, one all-to-all moves the photon records (LOCAL: one kernel launch; RCCL:
 *                  ncclSend / ncclRecv, resolved only for such a group), and each rank imports its slab and
 *                  gathers only the hit points inside it, so the per-pixel gather work divides by n.  The
 *                  host waits for the histogram copy's stream: the one host synchronisation per iteration
 *                  that SLABS adds to the pipelined schedule (ROWS photons have none in steady state).
 *                  The send and receive buffers are sized from the plan's counts and grow on demand.  VCM
 *                  and PT run exactly as with ROWS photons, and so does n == 1 (one slab: nothing to
 *                  exchange).  SLABS needs the uniform grid: n > 1 with photon_map != 0 gives
 *                  ORX_ERR_UNSUPPORTED; SLABS with ORX_GROUP_BATCH (whole-frame ranks, nothing to
 *                  partition) and photon_partition > 1 give ORX_ERR_INVALID_ARGUMENT.
 * ORX_GROUP_BATCH  the reference's own distribution: the caller issues the calls of one renderer, render(i, i,
 *                  radius_i) for i = 0, 1, 2, ...; global iteration i goes to rank i % n with that rank's own
 *                  local iteration count (the caller's local_iteration_number does not route; 0 restarts the
 *                  accumulation on every rank).  Each rank is a whole-frame renderer seeded by the batch seed
 *                  below.  A call only enqueues work, so n consecutive calls run on n devices side by side
 *                  (the calls that block the host on one renderer, such as the first frames after a resize,
 *                  block here too).  The merged image is the sum of the ranks' running sums, refreshed every
 *                  reduce_every local iterations of a rank and by the output call, which overwrites it:
 *                  reading the output changes nothing a later call returns.
 * Communicators: ORX_COMM_LOCAL, every rank on one device in one process (tests, development, a preview
 * with little memory): device-to-device copies and sums in rank order 0..n-1 in fp32, deterministic and
 * equal to a sequential float32 sum on the host.  ORX_COMM_RCCL: librccl opened with dlopen when selected
 * (ORX_ERR_UNSUPPORTED with the loader's message when it is missing; ORX_RCCL_LIB names another file), one
 * communicator per rank.  ORX_COMM_AUTO: LOCAL when all ranks share a device, RCCL otherwise.
 * Arguments are checked before the first HIP call: n == 0, n > 64, hip_devices or out NULL, a negative device,
 * an unknown enum value: ORX_ERR_INVALID_ARGUMENT; LOCAL with ranks on different devices (or RCCL with
 * several ranks on one): ORX_ERR_UNSUPPORTED; no device present: ORX_ERR_DEVICE.  cfg or the group config
 * NULL: the defaults.  *out is NULL after any failure, and the message of a failed creation is returned by
 * the last-error call on a NULL group (per thread).  Errors are kept per group; a rank's failure is copied
 * with "rank k: " in front. */
typedef struct orx_group orx_group;
typedef enum { ORX_GROUP_BATCH = 0, ORX_GROUP_ROWS = 1 } orx_group_partition;
typedef enum { ORX_COMM_AUTO = 0, ORX_COMM_LOCAL = 1, ORX_COMM_RCCL = 2 } orx_group_comm;
typedef enum { ORX_PHOTONS_ROWS = 0, ORX_PHOTONS_SLABS = 1 } orx_group_photons;
typedef struct {
    uint32_t partition;     /* orx_group_partition */
    uint32_t comm;          /* orx_group_comm */
    uint32_t reduce_every;  /* BATCH: merge the running sums every K local iterations of a rank; 0: only on get_output. default 8 */
    uint32_t pipeline;      /* ROWS + PPM: 1 (default) the pipelined schedule, 0 serial phases */
    uint32_t photon_partition; /* orx_group_photons; ROWS + PPM: whose photons a rank gathers against. default ROWS */
    uint32_t reserved[3];
} orx_group_config;

void orx_default_group_config(orx_group_config* cfg);
orx_status orx_create_group(uint32_t n, const int* hip_devices, const orx_config* cfg, const orx_group_config* group_cfg,
                            orx_group** out);
orx_status orx_group_init_scene(orx_group* g, const orx_scene* scene);
/* a change of details->width / height behaves as on one renderer; the exchange buffers follow it */
orx_status orx_group_render_next_iteration(orx_group* g, uint64_t iteration_number, uint64_t local_iteration_number,
                                           float ppm_radius, int create_output, const orx_request* details);
/* the full W*H*3 running sum, synchronous: an outstanding pipelined finish is drained first; ROWS: the ranks'
 * rows de-interleaved on the device; BATCH: the merged sum */
orx_status orx_group_get_output(orx_group* g, float* dst, size_t dst_bytes);
/* The group's convergence statistics and display image (see orx_set_convergence above; same arguments).  ROWS:
 * every rank keeps the statistics of its rows; the query computes each rank's error and mean-luminance planes,
 * all-gathers them, assembles global rows on rank 0 and reduces the tiles there, after finishing an
 * outstanding pipelined iteration as orx_group_get_output does.  BATCH: orx_group_set_convergence returns
 * ORX_ERR_UNSUPPORTED (the ranks' windows would have to be merged).  orx_group_get_display builds the merged
 * image as orx_group_get_output does, in both partitions, and converts it on rank 0: W*H*4 bytes. */
orx_status orx_group_set_convergence(orx_group* g, int enable);
orx_status orx_group_get_convergence(orx_group* g, float floor, float threshold, orx_convergence* out,
                                     float* tile_error, size_t tile_bytes);
orx_status orx_group_get_display(orx_group* g, float inv_iterations, float inv_gamma, int32_t format,
                                 uint8_t* dst, size_t dst_bytes);
uint32_t orx_group_world(const orx_group* g);
/* borrowed (stats, buffers); owned by the group */
orx_renderer* orx_group_renderer(orx_group* g, uint32_t rank);
/* 1 if the last iteration ran the pipelined ROWS PPM schedule */
int orx_group_pipelined(const orx_group* g);
/* "local" or "rccl" */
const char* orx_group_comm_name(const orx_group* g);
const char* orx_group_last_error(const orx_group* g);
void orx_group_destroy(orx_group* g);
/* Rank's RNG seed in the BATCH partition (pure): rank 0 keeps `seed`, so a one-rank group renders the
 * single-device sequence; with seed 0 the others fold clock_ns to 32 bits (t ^ t >> 32) first; then
 * seed + 0x9E3779B9 rank mod 2^32, and 1 in place of 0 */
uint32_t orx_batch_seed(uint32_t seed, uint32_t rank, uint64_t clock_ns);
/* inspection: the LOCAL communicator's sum collectives on host arrays (staged through the device).
 * in [world][world * block_floats] -> out [world][block_floats]; in [world][n_floats] -> out [n_floats] */
orx_status orx_group_debug_reduce_scatter(orx_group* g, const float* in, size_t block_floats, float* out);
orx_status orx_group_debug_reduce(orx_group* g, const float* in, size_t n_floats, float* out);
/* The slab planner (pure, host only: no renderer and no device; multigpu.slab_plan's voxel form with its
 * default weights, in double precision).  hists: the ranks' orx_ppm_slab_histogram outputs back to back,
 * [world][orx_slab_histogram_words(nbins)]; halo_bins: one per axis (orx_ppm_slab_halo; NULL: 0).  A bin's
 * cost mixes the gather (its hit points, each weighted by the photon count of its voxel), the import
 * (photons) and the per-pixel work (hit points), 0.8 / 0.15 / 0.05, each normalised to sum 1; on each axis a
 * bin goes to rank min(floor(mid world / total), world - 1), mid the cumulative cost at the bin's midpoint
 * (an even split of the bins when the total is 0); the axis with the smallest largest-slab cost wins, ties
 * the lower axis.  Writes *axis, bin_dest[nbins] (ascending), counts[world][world] (records rank s sends to
 * rank d: a photon in bin b goes to every rank from bin_dest[b - halo] to bin_dest[b + halo], clamped) and
 * photon_box[6] (the min / max over ranks of the histograms' AABB words; NULL: not wanted).  world 1..64,
 * nbins a multiple of ORX_SLAB_VOXELS and at most 1024, no NULL among the others: ORX_ERR_INVALID_ARGUMENT. */
orx_status orx_slab_plan(const uint32_t* hists /* [world][orx_slab_histogram_words(nbins)] */, uint32_t world,
                         uint32_t nbins, const uint32_t halo_bins[3], uint32_t* axis, uint8_t* bin_dest /* [nbins] */,
                         uint64_t* counts /* [world][world]: records s sends to d */, uint32_t photon_box[6]);
/* the plan of the group's last SLABS iteration (1024 bins): ORX_ERR_STATE when there was none (ROWS photons,
 * n == 1, no PPM iteration yet) */
orx_status orx_group_slab_plan(const orx_group* g, uint32_t* axis, uint8_t* bin_dest /* [1024] */,
                               uint64_t* counts /* [n][n] */);
/* inspection: the LOCAL communicator's all-to-all of photon records (36 bytes each) on host arrays, staged
 * through the device like orx_group_debug_reduce.  counts[n][n] in records: rank s sends counts[s][d] to d.
 * in  = rank 0's send buffer, rank 1's, ...; rank s's buffer holds its records for d = 0..n-1 back to back.
 * out = rank 0's receive buffer, rank 1's, ...; rank d's holds what s = 0..n-1 sent, back to back. */
orx_status orx_group_debug_all_to_all(orx_group* g, const float* in, const uint64_t* counts, float* out);

/* ---- Checkpoint / resume ----
 * What survives an iteration of a progressive render is the running sum, the RNG buffer and the numbers of
 * the last iteration; a state blob holds exactly that, so that a render can be saved, ended, and continued
 * by another process, or by another number of devices: an RNG slot's chain does not depend on the rank that
 * owns the slot (orx_set_shard), so one canonical frame serves a single renderer and a ROWS group of any
 * world.  Everything else (photon maps, hit points, light vertices, the grid schedule's probe) is rebuilt by
 * the next iteration.  One exception: with a medium box active the next eye pass gathers the volumetric
 * photon table of the previous photon pass, which is not part of the blob: such a renderer does not save.
 *
 * A blob is a 128-byte little-endian header and two payload sections:
 *   offset size
 *        0    8  magic "ORXSTATE"
 *        8    4  format version (1)
 *       12    4  header bytes (128)
 *       16    8  total bytes (header + sections)
 *       24    4  kind: 0 a frame, 1 a BATCH container
 *       28    4  flags: bit 0, the VCM subpath-length estimate has run for this size
 *       32    4  W                    36    4  H
 *       40    4  rng_width = max(photon_launch_width, W)
 *       44    4  rng_height = max(photon_launch_height, H)
 *       48    4  photon_launch_width  52    4  photon_launch_height
 *       56    4  method (orx_method) of the last completed iteration
 *       60    4  its ppm_radius (float)
 *       64    8  its iteration_number
 *       72    8  its local_iteration_number
 *       80    8  scene key (orx_scene_key)
 *       88    4  world (containers; 0 in a frame)
 *       92    4  reserved, 0
 *       96    8  calls (containers: the group's iterations since the last restart; 0 in a frame)
 *      104    8  FNV-1a 64 of section A
 *      112    8  FNV-1a 64 of section B
 *      120    8  FNV-1a 64 of header bytes 0..119
 *   frame:     A = RNG [rng_height][rng_width][6] uint32, global row order, words v0..v4, d (ORX_BUF_RNG);
 *              B = output [H][W][3] float, the running sum (orx_get_output)
 *   container: A = `world` frames back to back, rank 0 first, each with its rank's own local iteration
 *              count in its header; B is empty
 * The checksums reject truncated or damaged files; they authenticate nothing.
 *
 * The four calls below are pure (host only: no renderer and no device).  orx_state_info_read checks magic,
 * version, sizes (with overflow-safe arithmetic, before anything is read with them) and the three checksums,
 * and never reads past `bytes`; bytes beyond the blob's total are ignored.  Any defect, a NULL argument:
 * ORX_ERR_INVALID_ARGUMENT.  orx_state_packed_bytes: the size of a frame with the info's dimensions (0 when
 * they are not a frame's: a zero size, rng smaller than the image, an overflow, kind 1).  orx_state_pack writes
 * a frame (version, total size, world and calls of `info` are ignored).  orx_state_unpack checks as
 * orx_state_info_read does and returns views into the blob (a container: *rng is its first frame's header,
 * *output NULL). */
typedef struct {
    uint32_t version;               /* 1 */
    uint32_t kind;                  /* 0 frame, 1 BATCH container */
    uint32_t flags;                 /* bit 0: VCM estimate has run */
    uint32_t width, height;
    uint32_t rng_width, rng_height;
    uint32_t photon_launch_width, photon_launch_height;
    int32_t method;                 /* orx_method */
    float ppm_radius;
    uint32_t world;                 /* containers */
    uint64_t iteration_number;
    uint64_t local_iteration_number;
    uint64_t scene_key;
    uint64_t calls;                 /* containers */
    uint64_t total_bytes;
} orx_state_info;
orx_status orx_state_info_read(const void* blob, size_t bytes, orx_state_info* out);
size_t orx_state_packed_bytes(const orx_state_info* info);
orx_status orx_state_pack(const orx_state_info* info, const uint32_t* rng, const float* output, void* dst,
                          size_t dst_bytes);
orx_status orx_state_unpack(const void* blob, size_t bytes, const uint32_t** rng, const float** output);
/* FNV-1a 64 over the contents of a scene as orx_init_scene deep-copies it, in field order: each count, then
 * per array one byte (1 present, 0 NULL or empty) and its elements; materials and lights as their structs
 * (4-byte fields, no padding); textures as width, height, texels, normal map; pointer values never enter.
 * Pure; NULL gives 0. */
uint64_t orx_scene_key(const orx_scene* scene);

/* Save and restore on one renderer.  orx_state_bytes: the size of its frame blob, 0 before the first frame.
 * orx_save_state is synchronous: it finishes what is outstanding (the pipelined PPM gather, the overlapped
 * VCM resolve), copies the RNG planes and the sum to the host and packs them; nothing a later call returns
 * changes.  Before the first frame: ORX_ERR_STATE; with a medium box active: ORX_ERR_UNSUPPORTED (above).
 * orx_restore_state (after orx_init_scene; before it ORX_ERR_STATE) checks the blob, its scene key and photon
 * launch size against the renderer's (ORX_ERR_INVALID_ARGUMENT, the message names both values), then does
 * what a request of the blob's W x H would do on arrival, except that the RNG is loaded, not seeded: the
 * frame is sized, the sum loaded, the pixel size factor and the estimate flag set.  The next
 * orx_render_next_iteration of that size with local_iteration_number != 0 continues the sum (0 clears it and
 * keeps the loaded RNG; another size resizes and seeds, as ever).  The loaded RNG stands in for cfg.seed: a
 * clock-seeded render resumes exactly.  A renderer sharded with orx_set_shard (world > 1): both calls give
 * ORX_ERR_UNSUPPORTED (a group saves and restores its ranks' rows itself, below). */
size_t orx_state_bytes(const orx_renderer* r);
orx_status orx_save_state(orx_renderer* r, void* dst, size_t dst_bytes);
orx_status orx_restore_state(orx_renderer* r, const void* blob, size_t bytes);

/* Render groups.  ROWS (either photon partition): the blob is a frame, byte for byte that of one renderer, so
 * a save from one renderer restores into a ROWS group of any world and back; each rank moves its own rows
 * (global row rank + j world <-> local row j), de-interleaved on the device when the ranks share one, copied
 * row by row through the host otherwise.  BATCH: a container of the ranks' frames; restore needs the same
 * world (ORX_ERR_INVALID_ARGUMENT otherwise, and for a frame into a BATCH group or a container into a ROWS
 * group or a renderer); the merged image is rebuilt by the next reduce or output call.  Save drains an
 * outstanding pipelined finish, as orx_group_get_output does.  orx_group_state_bytes: 0 before the first
 * frame. */
size_t orx_group_state_bytes(const orx_group* g);
orx_status orx_group_save_state(orx_group* g, void* dst, size_t dst_bytes);
orx_status orx_group_restore_state(orx_group* g, const void* blob, size_t bytes);

#ifdef __cplusplus
}
#endif

#endif /* ORX_H */
