/*
 * rt4.h — C ABI of the MI355X-native 4D path tracer (the drop-in boundary).
 *
 * The reference (BusyginIvan/4D_ray_tracing) has exactly one hot path: the per-cell trace loop of
 * executable/shader.frag (GLSL 330), driven by SFML through uniforms and one draw call per window.
 * This header replaces that boundary with plain C: POD structs, pointers and sizes, int status codes.
 *
 * Reference interface each entry point replaces (paths relative to the reference root):
 *   rt4_uniforms                  <- the 13 GLSL uniforms, executable/shader.frag:5-19, set through
 *                                    sf::Shader::setUniform in src/main.cpp:28-38,86-91 and
 *                                    src/windows/windows.cpp:41-44
 *   rt4_scene_desc                <- the scene block pasted into shader.frag (shader.frag:412-451,
 *                                    scenes/<name>.frag) + optional final_light override (shader.frag:454-468)
 *   rt4_scene_load_frag/parse     <- "paste a scene over shader.frag" workflow (executable/README.md:9-11),
 *                                    compiled at run time by sf::Shader::loadFromFile (src/main.cpp:26)
 *   rt4_properties_*              <- Properties (inc/properties.h:8-18, src/properties.cpp:12-77)
 *   rt4_orientation_update        <- Orientation::update (src/controls.cpp:72-86)
 *   rt4_uniforms_from_properties  <- initShader + first-frame uniforms (src/main.cpp:25-39,86-91),
 *                                    initControls (src/controls.cpp:140-159), CellsWindow
 *                                    (src/windows/windows.cpp:6-13,24-34)
 *   rt4_section_basis             <- ThreeWindowGroup::drawShaderImage (three_window_group.cpp:42-46)
 *   rt4_render_device / _host     <- CellsWindow::drawShaderImage -> texture.draw(sprite,&shader)
 *                                    (src/windows/windows.cpp:40-47): the "kernel launch"
 *
 * Conventions
 *   - Status: 0 = RT4_OK, negative = error; `err` (may be NULL) receives a NUL-terminated message.
 *     Nothing in the library aborts (the reference's error() aborts: src/util/util.cpp:9-12).
 *   - Images are float RGBA (16 B per pixel). Row 0 is the TOP of the displayed image, which in the
 *     reference is gl_FragCoord.y = 0.5 (RenderTexture::display() is never called).
 *   - The framebuffer is read (old_frame) and written in place by the lane that owns the pixel.
 *   - Re-entrant per (context, stream). One context per device per host thread.
 */
#ifndef RT4_H
#define RT4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT4_ABI_VERSION 2

enum rt4_status {
  RT4_OK = 0,
  RT4_ERR_ARG = -1,      /* bad argument / out-of-range value */
  RT4_ERR_IO = -2,       /* file cannot be opened or read */
  RT4_ERR_PARSE = -3,    /* properties or scene text not understood */
  RT4_ERR_HIP = -4,      /* HIP runtime error (no device, launch failure, ...) */
  RT4_ERR_CAPACITY = -5, /* scene exceeds the RT4_MAX_* limits below */
  RT4_ERR_PROPERTY = -6  /* missing key / bad value (reference: Properties::get* error paths) */
};

/* ---- uniforms: executable/shader.frag:5-19 (field-for-field) ------------------------------- */
typedef struct rt4_uniforms {
  int32_t seed;               /* shader.frag:5   (main.cpp:86, time based there; fixed here)    */
  int32_t samples;            /* shader.frag:6   ray_tracing.samples                          */
  int32_t reflections_amount; /* shader.frag:7   ray_tracing.reflections_amount               */
  float small_indent;         /* shader.frag:8   ray_tracing.small_indent                     */
  float resolution[2];        /* shader.frag:10  cells (windows.cpp:41)                       */
  float part;                 /* shader.frag:12  1/frameNumber (main.cpp:87)                  */
  float light_to_color_conversion_coefficient; /* shader.frag:13                            */
  float mtr_sizes[2];         /* shader.frag:16  (matrix_height*GOLDEN, matrix_height)        */
  float focus[4];             /* shader.frag:17                                               */
  float vec_to_mtr[4];        /* shader.frag:18  forward * focus_to_matrix_distance           */
  float top_drct[4];          /* shader.frag:19                                               */
  float right_drct[4];        /* shader.frag:19                                               */
} rt4_uniforms;

/* ---- scene: the primitive types of shader.frag:163-400 --------------------------------------- */
typedef struct rt4_material { /* shader.frag:163-167 */
  float glow;
  float refl_prob;
  float color[3];
} rt4_material;

typedef struct rt4_space { /* visible_space, shader.frag:225-228 */
  float point[4];
  float norm[4];
  rt4_material material;
} rt4_space;

typedef struct rt4_sphere { /* visible_sphere, shader.frag:189-192 */
  float center[4];
  float r;
  rt4_material material;
} rt4_sphere;

typedef struct rt4_cylinder { /* visible_cylinder, shader.frag:243-247 */
  float point[4];
  float axis1[4];
  float axis2[4];
  float r;
  rt4_material material;
} rt4_cylinder;

typedef struct rt4_cylinders_union { /* visible_cylinders_union, shader.frag:279-281 */
  rt4_cylinder cylinder1, cylinder2;
} rt4_cylinders_union;

typedef struct rt4_tiger { /* visible_tiger, shader.frag:298-300 (built by init_tiger :303-314) */
  rt4_cylinder inner_cyl1, outer_cyl1, inner_cyl2, outer_cyl2;
} rt4_tiger;

typedef struct rt4_cube { /* visible_cube, shader.frag:345-350 */
  float point[4]; /* space.point */
  float norm[4];  /* space.norm  */
  float x[4], y[4], z[4];
  float r;
  rt4_material material;
} rt4_cube;

typedef struct rt4_hypercube { /* visible_hypercube, shader.frag:370-372 (init_hypercube :374-392) */
  rt4_cube cubes[8];
} rt4_hypercube;

typedef struct rt4_sun { /* sun_properties, shader.frag:404-409 */
  float drct[4];
  float angular_size;
  float light[3];
  float sharpness;
} rt4_sun;

/* One statement `inter = closest(<group>_intersection(...), inter);` of find_intersection
 * (shader.frag:434-451). Groups are tested in array order; ties keep the accumulated hit. */
enum rt4_group_kind {
  RT4_GROUP_SPACES = 1,           /* for (i) space_intersection(spaces[i], ray)            :437-438 */
  RT4_GROUP_SPHERES = 2,          /* for (i) sphere_intersection(spheres[i], ray, outer)   :440-441 */
  RT4_GROUP_CYLINDERS = 3,        /* for (i) cylinder_intersection(cylinders[i], ray, outer) :443-444 */
  RT4_GROUP_CYLINDERS_UNION = 4,  /* cylinders_union_intersection(u, ray)                   :446 */
  RT4_GROUP_HYPERCUBE = 5,        /* hypercube_intersection(h, ray)                         :447 */
  RT4_GROUP_TIGER = 6             /* tiger_intersection(t, ray)                             :448 */
};

typedef struct rt4_group {
  int32_t kind;      /* rt4_group_kind */
  int32_t first;     /* index of the first object in the kind's array */
  int32_t count;     /* objects tested by this statement (1 for union/hypercube/tiger) */
  int32_t outer;     /* `outer` argument of sphere/cylinder tests (shader.frag:197,251) */
  int32_t new_first; /* 1: closest(new, inter) (reference form: tie keeps inter);
                        0: closest(inter, new) (tie takes the new hit) */
} rt4_group;

#define RT4_MAX_GROUPS 16
#define RT4_MAX_SPACES 32
#define RT4_MAX_SPHERES 32
#define RT4_MAX_CYLINDERS 16
#define RT4_MAX_UNIONS 4
#define RT4_MAX_HYPERCUBES 4
#define RT4_MAX_TIGERS 4

enum rt4_final_light_mode {
  RT4_FINAL_LIGHT_SUN_SKY = 0, /* default final_light, shader.frag:454-468 */
  RT4_FINAL_LIGHT_CONSTANT = 1 /* override returning a constant vec3 (S-room: scenes/Комната...:38-40) */
};

typedef struct rt4_scene_desc {
  float sky_light[3];         /* shader.frag:414 */
  rt4_sun sun;                /* shader.frag:415 */
  int32_t final_light_mode;   /* rt4_final_light_mode */
  float final_light_const[3]; /* value returned by a constant override */
  int32_t n_groups;
  rt4_group groups[RT4_MAX_GROUPS];
  int32_t n_spaces;
  rt4_space spaces[RT4_MAX_SPACES];
  int32_t n_spheres;
  rt4_sphere spheres[RT4_MAX_SPHERES];
  int32_t n_cylinders;
  rt4_cylinder cylinders[RT4_MAX_CYLINDERS];
  int32_t n_unions;
  rt4_cylinders_union unions[RT4_MAX_UNIONS];
  int32_t n_hypercubes;
  rt4_hypercube hypercubes[RT4_MAX_HYPERCUBES];
  int32_t n_tigers;
  rt4_tiger tigers[RT4_MAX_TIGERS];
} rt4_scene_desc;

/* ---- library info ------------------------------------------------------------------------- */
int rt4_abi_version(void);
const char* rt4_build_info(void); /* "rt4 <ver> gfx950 hip <ver> ..." */
size_t rt4_scene_desc_size(void); /* sizeof(rt4_scene_desc), for binding-layout checks */
size_t rt4_uniforms_size(void);

/* ---- properties.txt (src/properties.cpp:12-77) --------------------------------------------- */
typedef struct rt4_properties rt4_properties;
int rt4_properties_load(const char* path, rt4_properties** out, char* err, size_t errlen);
int rt4_properties_parse(const char* text, size_t len, rt4_properties** out, char* err, size_t errlen);
void rt4_properties_free(rt4_properties* p);
int rt4_properties_has(const rt4_properties* p, const char* key);
/* getString: copies the value (truncated to buflen-1); *needed receives strlen(value) if non-NULL */
int rt4_properties_get_string(const rt4_properties* p, const char* key, char* buf, size_t buflen,
                              size_t* needed, char* err, size_t errlen);
int rt4_properties_get_int(const rt4_properties* p, const char* key, int32_t* out, char* err, size_t errlen);
int rt4_properties_get_uint(const rt4_properties* p, const char* key, uint32_t* out, char* err, size_t errlen);
int rt4_properties_get_float(const rt4_properties* p, const char* key, float* out, char* err, size_t errlen);
int rt4_properties_get_bool(const rt4_properties* p, const char* key, int* out, char* err, size_t errlen);

/* ---- camera (src/controls.cpp:64-86) ------------------------------------------------------- */
typedef struct rt4_orientation {
  float forward[4], top[4], right[4], w_drct[4];
  float horizontal_forward[4], horizontal_right[4], vertical_top[4];
} rt4_orientation;
/* angles in radians (the reference converts degrees with convertDegreesToRadians, math.cpp:29) */
void rt4_orientation_update(float fi, float te, float psi, rt4_orientation* out);

enum rt4_section { /* three_window_group.cpp:42-46 */
  RT4_SECTION_YXZ = 0, /* main window:  top_drct = top,    right_drct = right */
  RT4_SECTION_YWZ = 1, /* extra window: top_drct = top,    right_drct = w     */
  RT4_SECTION_YXW = 2  /* extra window: top_drct = w,      right_drct = right */
};
int rt4_section_basis(const rt4_orientation* o, int section, float top[4], float right[4]);

/* Builds every uniform the reference host sets for the first frame of a still camera:
 * samples/reflections/indent/k/mtr_sizes (main.cpp:28-38), focus + vec_to_mtr (main.cpp:88-91,
 * controls.cpp:151-158), top/right for `section` and resolution = cells (windows.cpp:41-44),
 * part = 1 (frameNumber 1), seed = 0. cells_w/cells_h are the render resolution. */
int rt4_uniforms_from_properties(const rt4_properties* p, int32_t cells_w, int32_t cells_h, int section,
                                 rt4_uniforms* out, rt4_orientation* orientation_out, char* err,
                                 size_t errlen);
/* cells of a window: width/cell_size, (width/GOLDEN)/cell_size (windows.cpp:6-13,25-26);
 * window_type is "main" or "additional" (keys window.<type>.width / .cell_size). */
int rt4_window_cells(const rt4_properties* p, const char* window_type, int32_t* cells_w, int32_t* cells_h,
                     char* err, size_t errlen);

/* ---- camera model: SphOrientation, mouse / wheel / WASD-EQ motion (src/controls.cpp) ---------- */
typedef struct rt4_camera {
  float fi, te, psi;                       /* radians, normalised (SphOrientation, controls.cpp:25-54) */
  float psi_range_center, psi_range_radius;
  int32_t constrain_psi_range;
  float mouse_sensitivity, wheel_sensitivity, movement_speed; /* controls.cpp:144-147 */
  float focus_to_matrix_distance;          /* main.cpp:73 */
  float focus[4];                          /* controls.cpp:150-156 */
  uint32_t frame_number;                   /* frames since the camera last changed, from 1 (main.cpp:72) */
  rt4_orientation orientation;             /* Orientation::update() of (fi, te, psi) */
} rt4_camera;

/* Movement keys held during a frame (controls.cpp:98-113). */
enum rt4_move_key {
  RT4_KEY_FORWARD = 1,  /* W      horizontal_forward */
  RT4_KEY_BACK = 2,     /* S     -horizontal_forward */
  RT4_KEY_RIGHT = 4,    /* D      horizontal_right   */
  RT4_KEY_LEFT = 8,     /* A     -horizontal_right   */
  RT4_KEY_UP = 16,      /* Space  vertical_top       */
  RT4_KEY_DOWN = 32,    /* LShift -vertical_top      */
  RT4_KEY_W_POS = 64,   /* E      w_drct             */
  RT4_KEY_W_NEG = 128   /* Q     -w_drct             */
};

/* initControls + SphOrientation::init (controls.cpp:140-159, :29-39): angles from degrees, psi range,
 * sensitivities, speed, focus; frame_number = 1. */
int rt4_camera_init(const rt4_properties* p, rt4_camera* cam, char* err, size_t errlen);
/* changeFi / changeTe / changePsi (each re-normalises) + Orientation::update + frame_number = 1
 * (controls.cpp:51-53, :186-198). */
void rt4_camera_rotate(rt4_camera* cam, float d_fi, float d_te, float d_psi);
/* Event::MouseMoved with the cursor (dx, dy) from the window centre, dy up (controls.cpp:181-193):
 * returns 1 and changes nothing when |dx| or |dy| exceeds max_offset (the cursor is re-centred),
 * 0 after rotating by (dx, dy) * mouse_sensitivity (a zero move changes nothing). */
int rt4_camera_mouse_move(rt4_camera* cam, int32_t dx, int32_t dy, uint32_t max_offset);
/* Event::MouseWheelScrolled: psi += delta * wheel_sensitivity (controls.cpp:196-201). */
void rt4_camera_wheel(rt4_camera* cam, float delta);
/* move(seconds) (controls.cpp:118-134): focus += drct * (seconds * movement_speed / |drct|) for the
 * sum drct of the held keys' directions; frame_number = 1 when it moved. */
void rt4_camera_move(rt4_camera* cam, uint32_t keys, float seconds);
/* Uniforms of the next frame (main.cpp:86-91, windows.cpp:41-44): base supplies samples,
 * reflections_amount, small_indent, k, mtr_sizes and resolution; then seed, part = 1/frame_number,
 * focus, vec_to_mtr = forward * focus_to_matrix_distance and top/right of `section`. Advances
 * frame_number (frameNumber++). */
int rt4_camera_frame_uniforms(rt4_camera* cam, const rt4_uniforms* base, int section, int32_t seed,
                              rt4_uniforms* out);

/* ---- image output (presentation; windows.cpp:24-53 shows frames in SFML windows instead) ------ */
/* Binary PPM (P6) of an RGBA frame in any rt4_frame_format, rows top first, alpha dropped; float
 * channels are clamped to [0, 1] and mapped with the RGBA8 rule u = (uint8)(v * 255 + 0.5). */
int rt4_write_ppm(const char* path, const void* frame, int32_t format, int32_t w, int32_t h, int64_t row_stride_px,
                  char* err, size_t errlen);
/* The same pixels as an 8-bit RGB PNG (uncompressed deflate blocks, so no zlib dependency); w <= 21844. */
int rt4_write_png(const char* path, const void* frame, int32_t format, int32_t w, int32_t h, int64_t row_stride_px,
                  char* err, size_t errlen);

/* ---- accumulator checkpoint / resume (no reference counterpart) ----------------
 * The reference keeps the progressive average only in the window's texture: old_frame is blended with
 * part = 1/frameNumber (main.cpp:86-91) and restarts at frameNumber = 1 when the camera moves
 * (controls.cpp:132,181,190). A checkpoint is that texture in its rt4_frame_format plus the number of
 * frames already blended and the base seed, so a resumed run (frames frames_done + 1, ... through
 * rt4_progressive_uniforms) continues the same blend bit for bit.
 * File (little-endian): "RT4ACC1\0", int32 version (2), w, h, format, int64 frames_done, uint32 seed,
 * uint32 key (rt4_accum_key of the run, 0 = not recorded; version-1 files hold 0 there and still load),
 * then h rows of w pixels, rows top first, no padding. A save writes <path>.tmp, flushes it to the disk and
 * renames it over path, so a failed save leaves the previous checkpoint intact. */
#define RT4_ACCUM_VERSION 2
int rt4_accum_save(const char* path, const void* frame, int32_t format, int32_t w, int32_t h, int64_t row_stride_px,
                   int64_t frames_done, uint32_t seed, char* err, size_t errlen);
/* rt4_accum_save with the run's key, so that a resume can refuse a checkpoint of another run. */
int rt4_accum_save_key(const char* path, const void* frame, int32_t format, int32_t w, int32_t h, int64_t row_stride_px,
                       int64_t frames_done, uint32_t seed, uint32_t key, char* err, size_t errlen);
/* The run's key (never 0): a hash of the scene and of the uniforms that decide the progressive image other
 * than seed and part (samples, bounces, indent, tone-map coefficient, resolution, matrix, camera pose). */
uint32_t rt4_accum_key(const rt4_scene_desc* scene, const rt4_uniforms* u);
/* The key a checkpoint was saved with (0: not recorded). */
int rt4_accum_key_of(const char* path, uint32_t* key, char* err, size_t errlen);
/* Header only: any output pointer may be null. RT4_ERR_PARSE for a file that is not a checkpoint. */
int rt4_accum_info(const char* path, int32_t* w, int32_t* h, int32_t* format, int64_t* frames_done, uint32_t* seed,
                   char* err, size_t errlen);
/* Reads the pixels into a host frame of the checkpoint's w, h and format (RT4_ERR_ARG if the caller's
 * differ); the header fields as rt4_accum_info. */
int rt4_accum_load(const char* path, void* frame, int32_t format, int32_t w, int32_t h, int64_t row_stride_px,
                   int64_t* frames_done, uint32_t* seed, char* err, size_t errlen);

/* ---- scenes ------------------------------------------------------------------------------- */
/* Accepts a scene snippet (scenes/<name>.frag) or a whole shader.frag; UTF-8 paths. */
int rt4_scene_load_frag(const char* path, rt4_scene_desc* out, char* err, size_t errlen);
int rt4_scene_parse_frag(const char* text, size_t len, rt4_scene_desc* out, char* err, size_t errlen);
int rt4_scene_validate(const rt4_scene_desc* s, char* err, size_t errlen);
/* The reference's five scenes, rebuilt from their values (scenes/<name>.frag, executable/shader.frag):
 * "sphere" (Шар, плоскость и светилник), "room" (Комната со сферой), "tiger" (Фигура tiger; also
 * the shipped shader.frag default), "cylinder4d" (Четырёхмерный цилиндр), "hypercube" (Гиперкуб). */
int rt4_scene_builtin(const char* name, rt4_scene_desc* out, char* err, size_t errlen);

/* ---- surface index ---------------------------------------------------------
 * A flat numbering of everything a ray can hit, in the order of the arrays of rt4_scene_desc, whether or
 * not a group tests the object: spaces[i], spheres[i], cylinders[i], each unions[i] as cylinder1, cylinder2,
 * each hypercubes[i] as cubes[0..7], each tigers[i] as inner_cyl1, outer_cyl1, inner_cyl2, outer_cyl2.
 * rt4_gbuffer_px.surface holds this number. */
int32_t rt4_scene_surface_count(const rt4_scene_desc* s);
/* kind: rt4_group_kind of the owner; index: object in its kind's array; part: 0, or 0..1 / 0..7 / 0..3 inside a
 * union / hypercube / tiger. Any out pointer may be NULL. RT4_ERR_ARG for surface outside [0, count). */
int rt4_scene_surface(const rt4_scene_desc* s, int32_t surface, int32_t* kind, int32_t* index, int32_t* part,
                      rt4_material* material, char* err, size_t errlen);

/* ---- device context + trace kernel --------------------------------------------------------- */
typedef struct rt4_context rt4_context;

/* Memoise w_by_volume (shader.frag:141-150) over its whole input domain: rand() yields only
 * 2^23 values (shader.frag:111-118), so a 32 MiB table built on the device at context creation
 * by the same device function reproduces every Newton result bit for bit. */
#define RT4_FLAG_SAMPLER_LUT 0x1u
/* Always use the generic find_intersection (any group list) instead of the kernel specialised for
 * the scene's shape. Results are identical; used by the tests to cover both code paths. */
#define RT4_FLAG_GENERIC_KERNEL 0x2u
/* Primary-ray reuse. Every sample of a pixel starts with the same primary ray (shader.frag:519-521),
 * so find_intersection of that ray has the same result in all of them: the kernel evaluates it once
 * per pixel and starts every later sample from the cached candidate (shaded with the sample's own
 * random numbers, in the iteration that ended the previous sample). Images and the d_counter count
 * (find_intersection calls of the reference) are unchanged; rt4_context_evaluated reports the calls
 * actually evaluated. Specialised kernels only (ignored with RT4_FLAG_GENERIC_KERNEL or a generic
 * scene). SURVEY.md 8(d): a rate measured with it is labelled reference-equivalent. */
#define RT4_FLAG_PRIMARY_REUSE 0x4u
/* Overlapped launches (the default). A single-frame launch (rt4_render_device[_ex],
 * rt4_render_sections_device) runs its trace kernel on a context-owned side stream and writes the frame's light
 * sums to a context-owned slot buffer; only the blend into the frame (and the count) runs on the caller's stream.
 * Back-to-back frames (a moving camera, main.cpp:93; the 4D view's three sections, three_window_group.cpp:42-46)
 * then overlap each frame's trace with the previous frames' drain. Stream semantics are unchanged: the frame and
 * the counter are written in the caller's stream order; images and counts are identical to serial launches.
 * Depth and memory: a launch with fewer 8x8 tiles than the chip holds waves (~7000 tiles: the 4D view's sections
 * at properties.txt sizes) keeps up to 8 launches in flight on 8 side streams with 8 slot buffers; any larger one
 * up to 3, with 3 buffers. A slot buffer is 16 B per pixel of the largest launch it served: a 1080p frame uses
 * 3 x 33 MB, a 4K frame 3 x 133 MB, small frames at most 8 x 7.3 MB (rt4_context_overlap_bytes). The first launch
 * that needs a larger buffer waits on the host for the launches in flight and allocates it
 * (rt4_context_reserve_overlap does that ahead of time); if the allocation fails, that frame runs serially.
 * Hardware queues: the 8 side streams of the deep overlap share HIP's default four hardware queues per process;
 * set GPU_MAX_HW_QUEUES=8 in the environment before the process first touches HIP to give each its own (the 4D
 * view loop on config 2's scene: 0.25 ms per frame with the default, 0.17 ms with 8; frames that fill the chip
 * are unaffected). */
/* Every launch runs entirely on the caller's stream (no side streams, no slot buffers). */
#define RT4_FLAG_SERIAL_FRAMES 0x8u
/* Caps the overlap at 3 launches in flight for every frame size (3 side streams, 3 slot buffers): for processes
 * that keep HIP's four hardware queues or want the smaller footprint. Images and counts are unchanged. */
#define RT4_FLAG_OVERLAP_SHALLOW 0x10u

int rt4_context_create(int device, uint32_t flags, rt4_context** out, char* err, size_t errlen);
/* Uploads a scene (the reference recompiles the shader: src/main.cpp:25-39). Waits for the
 * context's launches still in flight on any stream before it replaces the device copy, so a frame
 * issued earlier renders the previous scene. Scene constants are verified on the device once per
 * process (cached by bit pattern), so setting a scene seen before costs only the upload. */
int rt4_context_set_scene(rt4_context* ctx, const rt4_scene_desc* scene, char* err, size_t errlen);
void rt4_context_destroy(rt4_context* ctx);

/* Pixel set of one launch (w <= 65535, h <= 16383). Local row i in [0,h) maps to image row
 *   band_rows == 0 : y0 + i
 *   band_rows  > 0 : y0 + (i / band_rows) * band_step + (i % band_rows)
 * and local column j in [0,w) to image column x0 + j. Scene coordinates come from the full image
 * size in uniforms.resolution, so any partition renders exactly the pixels of the whole image. */
typedef struct rt4_region {
  int32_t x0, y0, w, h;
  int32_t band_rows;
  int32_t band_step;
} rt4_region;

/* d_rgba: device float4 framebuffer; pixel (i, j) at d_rgba + 4*(i*row_stride_px + j).
 * Holds old_frame on entry and mix(old, new, part) on return (shader.frag:524-527).
 * d_counter (may be NULL): device uint64 incremented by the number of find_intersection calls
 * (one per ray-bounce, shader.frag:475). stream: hipStream_t (NULL = default stream).
 * Asynchronous: no host synchronisation and no allocation once the context's buffers hold the launch: the
 * tile-order buffer covers 2^18 8x8 tiles (16.7 M pixels; a larger launch grows it once) and the overlap's slot
 * buffers grow to the largest frame seen (without RT4_FLAG_SERIAL_FRAMES, the default: the first launch of a larger
 * frame waits for the launches in flight and allocates; rt4_context_reserve_overlap does it ahead of time; a
 * serial context has no slot buffers). Launches of one
 * context run in submission order: a launch on another stream than the previous one waits for it. */
int rt4_render_device(rt4_context* ctx, const rt4_uniforms* u, const rt4_region* region, float* d_rgba,
                      int64_t row_stride_px, unsigned long long* d_counter, void* stream, char* err,
                      size_t errlen);

/* Host-buffer convenience wrapper: copies rgba (same layout) to the device, renders, copies back,
 * synchronises. n_intersections (may be NULL) receives the count. */
int rt4_render_host(rt4_context* ctx, const rt4_uniforms* u, const rt4_region* region, float* rgba,
                    int64_t row_stride_px, uint64_t* n_intersections, char* err, size_t errlen);

/* ---- frame formats, progressive accumulation, batched sections --------- */
/* What old_frame / gl_FragColor live in. The blend mix(old, new, part) (shader.frag:524-527) is
 * always evaluated in fp32 (one fma per channel); only the stored value differs. */
enum rt4_frame_format {
  RT4_FRAME_RGBA32F = 0, /* float4, 16 B/pixel (rt4_render_device) */
  RT4_FRAME_RGBA16F = 1, /* IEEE half x4, 8 B/pixel: fp16 accumulator, stored round-to-nearest-even */
  RT4_FRAME_RGBA8 = 2    /* unorm8 x4, 4 B/pixel: the reference's RenderTexture (windows.cpp:31), which
                          * quantises old_frame every frame: old = u / 255.0f, stored
                          * u = (uint8_t)(min(max(v, 0), 1) * 255.0f + 0.5f), alpha 255 */
};
/* Bytes per pixel of a format; 0 if unknown. */
int32_t rt4_frame_format_bytes(int32_t format);

/* rt4_render_device for any frame format: d_frame holds h rows of row_stride_px pixels of the
 * format's size. */
int rt4_render_device_ex(rt4_context* ctx, const rt4_uniforms* u, const rt4_region* region, void* d_frame,
                         int32_t format, int64_t row_stride_px, unsigned long long* d_counter, void* stream,
                         char* err, size_t errlen);
int rt4_render_host_ex(rt4_context* ctx, const rt4_uniforms* u, const rt4_region* region, void* frame,
                       int32_t format, int64_t row_stride_px, uint64_t* n_intersections, char* err,
                       size_t errlen);

/* Progressive accumulation (main.cpp:72,86-88): frame_number counts frames since the camera last
 * moved, from 1. part = 1.0f / frame_number (frame 1 overwrites old_frame). The reference draws
 * a fresh time-based seed every frame (main.cpp:52-54,86); this deterministic replacement is
 * seed_n = base->seed ^ (frame_number * 0x9E3779B9). */
int rt4_progressive_uniforms(const rt4_uniforms* base, uint32_t frame_number, rt4_uniforms* out);

/* Up to three images in ONE launch: the sections of ThreeWindowGroup::drawShaderImage
 * (three_window_group.cpp:42-46; bases from rt4_section_basis). Per job: resolution, mtr_sizes,
 * vec_to_mtr, top_drct, right_drct, the region and the frame. seed, samples, reflections_amount,
 * small_indent, part, light_to_color_conversion_coefficient and focus must equal jobs[0]'s (one
 * shader, one frame; RT4_ERR_ARG otherwise). Each image equals its own rt4_render_device_ex bit for
 * bit; the pixel queue is shared, so the sections balance each other. Region h <= 16383 here. */
#define RT4_MAX_SECTIONS 3
typedef struct rt4_section_job {
  rt4_uniforms u;
  rt4_region region;
  void* d_frame;
  int64_t row_stride_px;
} rt4_section_job;
int rt4_render_sections_device(rt4_context* ctx, const rt4_section_job* jobs, int32_t n_jobs, int32_t format,
                               unsigned long long* d_counter, void* stream, char* err, size_t errlen);

/* n_frames consecutive frames into the same frame buffer, pipelined: the same result, bit for bit, as
 * n_frames calls of rt4_render_device_ex with u[0], u[1], ... in order (the frame loop of main.cpp:57-111
 * while the camera rests: progressive accumulation, or a benchmark loop), and d_counter receives the
 * sum of their counts. u[f] may differ from u[0] only in seed and part (rt4_progressive_uniforms);
 * RT4_ERR_ARG otherwise. The frames share one pixel queue (item = frame x 8x8 tile), so the drain at the
 * end of a launch (each lane finishing its last pixel's samples in order) is paid once per up to
 * RT4_MAX_FRAMES frames instead of once per frame. Each pixel's tone-mapped colour of every frame goes
 * to a context-owned scratch buffer (16 B per pixel and frame, up to 4 GiB: the frames are split into
 * launches that fit), then one pass blends the frames in order into d_frame with the same per-frame ops
 * and roundings as rt4_render_device_ex. The intermediate frames are not stored in d_frame. Regions
 * wider or taller than 8191 pixels run frame by frame. Asynchronous like rt4_render_device_ex; the first
 * call with a larger scratch need allocates (synchronises the stream once). */
#define RT4_MAX_FRAMES 64
int rt4_render_frames_device(rt4_context* ctx, const rt4_uniforms* u, int32_t n_frames, const rt4_region* region,
                             void* d_frame, int32_t format, int64_t row_stride_px, unsigned long long* d_counter,
                             void* stream, char* err, size_t errlen);
/* Allocates (and first-touches) the frame-colour scratch that pipelined launches of a w x h region use,
 * so that the first rt4_render_frames_device call of that size neither allocates nor synchronises.
 * Waits for the context's launches in flight when it has to grow the buffer. */
int rt4_context_reserve_frames(rt4_context* ctx, int32_t w, int32_t h, char* err, size_t errlen);
/* Frames per pipelined launch rt4_render_frames_device uses for a w x h region with the context's
 * current scene (1: frame by frame). The mirror-room tiger kernel (three or more spaces and a tiger)
 * runs frame by frame: it measured slower pipelined. */
int32_t rt4_context_frames_per_launch(const rt4_context* ctx, int32_t w, int32_t h);

/* ---- multi-GPU pixel bands (replaces the one whole-texture draw of windows.cpp:45) ---
 * A width x height frame is cut into bands of `band` rows (the last one may be short) dealt round-robin
 * over `world` ranks, so every rank gets the same mix of cheap sky rows and expensive object rows. Every
 * pixel is independent (shader.frag:104-108: the RNG depends only on the pixel, the seed and its own call
 * counter), so the assembled image equals a one-GPU render bit for bit.
 * rt4_band_plan: the region of `rank` (band layout of rt4_region; h = 0 when the rank owns no band) and
 * rows_max, the rows of the largest shard (>= 1): every rank renders into a buffer of rows_max rows of
 * width pixels, so one ncclGather of equal-size shards collects them (4d_ray_tracing_amd/shard.py
 * make_plan is the same arithmetic). RT4_ERR_ARG for width, height, world or band < 1, or rank outside
 * [0, world). */
int rt4_band_plan(int32_t width, int32_t height, int32_t world, int32_t band, int32_t rank, rt4_region* region,
                  int32_t* rows_max, char* err, size_t errlen);
/* Assembles the frame on the root from the gathered shards: d_gathered holds world x rows_max rows of
 * width pixels, rank-major (what ncclGather leaves on the root), d_image receives height rows of width
 * pixels (row stride width); pixel size rt4_frame_format_bytes(format). Asynchronous on stream (a
 * hipStream_t of the device that holds both buffers). */
int rt4_bands_unpermute_device(const void* d_gathered, void* d_image, int32_t width, int32_t height, int32_t world,
                               int32_t band, int32_t rows_max, int32_t format, void* stream, char* err, size_t errlen);

/* ---- primary-hit G-buffer, picking (no reference counterpart) ----------------
 * Every sample of a pixel starts with the same primary ray (shader.frag:519-521, no jitter), so the primary hit
 * is a noise-free function of the camera: one find_intersection per pixel gives it exactly. */
typedef struct rt4_gbuffer_px { /* 32 B */
  float normal[4];  /* the hit's normal exactly as find_intersection returns it; 0,0,0,0 on a miss */
  float depth;      /* the hit's dist (bits as returned, +inf and NaN hits included); +inf on a miss */
  int32_t surface;  /* surface index (rt4_scene_surface); -1 on a miss */
  float refl_prob;  /* the hit material's; 0 on a miss */
  float glow;       /* the hit material's; 0 on a miss */
} rt4_gbuffer_px;

/* The primary hit of every pixel of `region` with the context's scene: pixel (i, j) of the region at
 * d_gbuf + i*row_stride_px + j. One lane per pixel runs the trace kernel's primary-ray arithmetic and the
 * find_intersection of the context's selected kernel. Uses u's resolution, mtr_sizes, focus, vec_to_mtr, top_drct
 * and right_drct; ignores seed, samples, part and reflections_amount. Asynchronous on `stream`, no allocation, no
 * random numbers, nothing added to any intersection counter. Ordered with the context's other launches
 * (rt4_context_set_scene waits for it). d_gbuf must be 16-byte aligned (RT4_ERR_ARG otherwise). A pick is the
 * 1 x 1 region at the cursor. */
int rt4_render_gbuffer_device(rt4_context* ctx, const rt4_uniforms* u, const rt4_region* region, rt4_gbuffer_px* d_gbuf,
                              int64_t row_stride_px, void* stream, char* err, size_t errlen);
/* The same into a host buffer (synchronous; pixels outside the region keep their bytes). */
int rt4_render_gbuffer_host(rt4_context* ctx, const rt4_uniforms* u, const rt4_region* region, rt4_gbuffer_px* gbuf,
                            int64_t row_stride_px, char* err, size_t errlen);

/* ---- edge-stopping a-trous filter guided by the G-buffer ---------------------
 * For display only: the caller keeps its accumulator (the frame the renders blend into) and never passes the
 * filtered image back as old_frame. The frame and the G-buffer share the pixel indexing [0,w) x [0,h).
 * Definition (fp32 round-to-nearest, no contraction; the kernel matches it bit for bit):
 *   C_0 = the decoded input (float as stored, half -> float, u / 255.0f). p is filterable iff
 *   surface(p) >= 0 && refl_prob(p) <= max_refl_prob. For level l = 0 .. levels-1, s = 2^l, H = {1/16,1/4,3/8,1/4,1/16}:
 *   a pixel that is not filterable keeps C_l(p); a filterable p sums the taps dy = -2..2 (outer), dx = -2..2 (inner),
 *   q = p + s*(dx, dy); a tap counts iff q is inside the image and (q == p, or q is filterable, surface(q) ==
 *   surface(p), dot(n_p, n_q) >= cos_min (the fma chain of DESIGN.md §3) and fabsf(z_q - z_p) <= depth_tol * z_p);
 *   with k = H[dy+2]*H[dx+2]: acc_c = acc_c + k * C_l(q)_c (a multiply, then an add), wsum = wsum + k;
 *   C_{l+1}(p)_c = acc_c / wsum. The output is C_levels in the frame's format (half: round to nearest even; RGBA8:
 *   the rule of rt4_frame_format) with the input's stored alpha; a pixel that is not filterable gets the input's
 *   stored bits. */
#define RT4_DENOISE_MAX_LEVELS 6
typedef struct rt4_denoise_params {
  int32_t levels;      /* 1 .. RT4_DENOISE_MAX_LEVELS */
  float cos_min;       /* smallest dot of the two normals a tap may have */
  float depth_tol;     /* largest |z_q - z_p| a tap may have, as a fraction of z_p */
  float max_refl_prob; /* pixels whose primary hit reflects more often pass through unfiltered */
} rt4_denoise_params;
void rt4_denoise_params_default(rt4_denoise_params* p); /* 3, 0.9f, 0.1f, 0.5f */
/* d_in and d_out (w x h frames of `format`, row strides in pixels) must not overlap: RT4_ERR_ARG. Asynchronous on
 * `stream`. Intermediate levels and the repacked guide live in context-owned scratch (rt4_context_denoise_bytes):
 * the first call that needs more waits for the stream and allocates. Ordered with the context's other launches. */
int rt4_denoise_device(rt4_context* ctx, const void* d_in, int64_t in_stride_px, void* d_out, int64_t out_stride_px,
                       int32_t format, int32_t w, int32_t h, const rt4_gbuffer_px* d_gbuf, int64_t gbuf_stride_px,
                       const rt4_denoise_params* params, void* stream, char* err, size_t errlen);
/* The same on host buffers (synchronous; output pixels outside [0,w) x [0,h) keep their bytes). */
int rt4_denoise_host(rt4_context* ctx, const void* in, int64_t in_stride_px, void* out, int64_t out_stride_px,
                     int32_t format, int32_t w, int32_t h, const rt4_gbuffer_px* gbuf, int64_t gbuf_stride_px,
                     const rt4_denoise_params* params, char* err, size_t errlen);
/* Bytes of the context's denoise scratch (0 before the first rt4_denoise_device call). */
uint64_t rt4_context_denoise_bytes(const rt4_context* ctx);

/* ---- temporal reprojection (no reference counterpart) ------------------------
 * The reference restarts its progressive image whenever the camera moves (controls.cpp:132,181,190). Reprojection
 * carries every pixel's accumulated colour and its frame count (the history) to where its surface point appears in
 * the new view, and restarts only the pixels whose history is invalid. All images are whole frames [0,w) x [0,h);
 * u_cur->resolution and u_prev->resolution must equal (w, h). G_cur / G_prev are the G-buffers of u_cur / u_prev
 * (rt4_render_gbuffer_device), acc_prev / hist_prev the image and history of the old view.
 * Definition (fp32 round-to-nearest, no contraction, division and sqrt correctly rounded; dot is the fma chain of
 * DESIGN.md §3, mad(a,s,b) one fma per component; the kernel matches it bit for bit). For pixel p = (j, i), g = G_cur(p):
 *   1. p is eligible iff g.surface >= 0 && g.refl_prob <= max_refl_prob && fabsf(g.depth) < inf.
 *   2. d = the primary direction of p under u_cur, op for op as rt4_render_gbuffer_device builds it;
 *      X = mad(d, g.depth, focus_cur).
 *   3. v = X - focus_prev; F = vec_to_mtr_prev, T = top_drct_prev, R = right_drct_prev (assumed mutually orthogonal,
 *      T and R unit: every rt4_section_basis). a = dot(v,F) / dot(F,F), a > 0 required; t = dot(v,T), r = dot(v,R);
 *      e = mad(R, -r, mad(T, -t, mad(F, -a, v))), dot(e,e) <= (slice_tol*slice_tol) * dot(v,v) required (the 4D test:
 *      the point still lies in the 3D slice the old camera saw); dv = sqrt(dot(v,v)).
 *   4. mx = r / a, my = t / a; sx = mx / mtr_prev.x + 0.5f, sy = 0.5f - my / mtr_prev.y; fx = sx * res.x - 0.5f,
 *      fy = sy * res.y - 0.5f (a multiply, then a subtract); fx > -1 && fx < w && fy > -1 && fy < h required (false
 *      for NaN); x0 = floorf(fx), y0 = floorf(fy), ax = fx - x0, ay = fy - y0.
 *   5. Taps ty = 0,1 (outer), tx = 0,1 (inner): q = (x0+tx, y0+ty), k = (tx ? ax : 1-ax) * (ty ? ay : 1-ay). A tap
 *      counts iff q is inside the image, k > 0, hist_prev(q) > 0, G_prev(q).surface == g.surface,
 *      dot(n_p, n_q) >= cos_min and fabsf(dot(n_p, X_q - X)) <= plane_tol * dv, where X_q = mad(d_q, z_q, focus_prev),
 *      d_q the primary direction of q under u_prev and z_q = G_prev(q).depth (the distance of the old hit point from
 *      the new hit's tangent plane; a depth difference fails on surfaces seen at grazing angles). A counted tap adds
 *      acc_c = acc_c + k * C(q)_c (a multiply, then an add; C decoded as in the filter), wsum = wsum + k,
 *      nmin = min(nmin, hist_prev(q)).
 *   6. wsum > 0: the colour acc / wsum in the frame's format (fma(c, 1, 0), then half: round to nearest even; RGBA8:
 *      the rule of rt4_frame_format) with alpha 1, and hist_out = min(nmin, max_history). Every other case: the zero
 *      colour with alpha 1 and hist_out = 0. */
typedef struct rt4_reproject_params {
  float cos_min;       /* smallest dot(n_p, n_q) a tap may have */
  float plane_tol;     /* largest distance of the old hit point from the new hit's tangent plane, as a fraction of dv */
  float slice_tol;     /* largest out-of-slice distance of the hit point from the old camera's 3D slice, as a fraction of |v| */
  float max_refl_prob; /* pixels whose primary hit reflects more often restart */
  int32_t max_history; /* cap of the history length carried over (>= 1) */
} rt4_reproject_params;
/* 0.9f, 0.02f, 0.01f, 0.5f, 255. Starting points: nothing has been measured behind these values. */
void rt4_reproject_params_default(rt4_reproject_params* p);
/* Strides in elements of their image (G-buffer records, pixels, int32). RT4_ERR_ARG, nothing written, for a NULL
 * pointer, an unknown format, a resolution other than (w, h), a stride below w, a misaligned pointer (G-buffers 16 B,
 * frames their pixel size, histories 4 B), max_history < 1, or an output that overlaps an input or the other output.
 * Asynchronous on `stream`, no allocation. Ordered with the context's other launches. */
int rt4_reproject_device(rt4_context* ctx, const rt4_uniforms* u_cur, const rt4_gbuffer_px* d_gcur, int64_t gcur_stride,
                         const rt4_uniforms* u_prev, const rt4_gbuffer_px* d_gprev, int64_t gprev_stride,
                         const void* d_acc_prev, int64_t accp_stride, const int32_t* d_hist_prev, int64_t histp_stride,
                         void* d_acc_out, int64_t acco_stride, int32_t* d_hist_out, int64_t histo_stride, int32_t format,
                         int32_t w, int32_t h, const rt4_reproject_params* params, void* stream, char* err, size_t errlen);
/* The same on host buffers (synchronous; output bytes outside [0,w) x [0,h) keep their values). */
int rt4_reproject_host(rt4_context* ctx, const rt4_uniforms* u_cur, const rt4_gbuffer_px* gcur, int64_t gcur_stride,
                       const rt4_uniforms* u_prev, const rt4_gbuffer_px* gprev, int64_t gprev_stride, const void* acc_prev,
                       int64_t accp_stride, const int32_t* hist_prev, int64_t histp_stride, void* acc_out, int64_t acco_stride,
                       int32_t* hist_out, int64_t histo_stride, int32_t format, int32_t w, int32_t h,
                       const rt4_reproject_params* params, char* err, size_t errlen);

/* The progressive blend with a frame count per pixel. For every pixel: n = hist(p) + 1 (saturating at INT32_MAX;
 * hist(p) >= 0), part = 1.0f / (float)n, acc(p) = mix(acc(p), new(p).rgb, part) with the ops and roundings of
 * rt4_render_device_ex in `format` (alpha 1), hist(p) = n. d_new is RGBA32F: a frame rendered with part = 1 into a
 * buffer of finite values holds the tone-mapped colour itself, so with a uniform history this continues the plain
 * progressive image bit for bit. The three images must not overlap (RT4_ERR_ARG). Asynchronous, no allocation. */
int rt4_temporal_blend_device(rt4_context* ctx, const float* d_new_rgba32f, int64_t new_stride, void* d_acc,
                              int64_t acc_stride, int32_t format, int32_t* d_hist, int64_t hist_stride, int32_t w, int32_t h,
                              void* stream, char* err, size_t errlen);

/* The two together, with the state they need: two accumulators in `format`, two histories, two G-buffers, one RGBA32F
 * sample frame and the previous frame's uniforms, all allocated at creation (rt4_temporal_bytes). Destroy it before
 * its context. The scene must not change between frames: after rt4_context_set_scene call rt4_temporal_reset. */
typedef struct rt4_temporal rt4_temporal;
int rt4_temporal_create(rt4_context* ctx, int32_t w, int32_t h, int32_t format, rt4_temporal** out, char* err, size_t errlen);
void rt4_temporal_destroy(rt4_temporal* t); /* waits for the context's launches in flight */
/* The next frame starts over (history 0), as the first frame after creation does. */
void rt4_temporal_reset(rt4_temporal* t);
/* One frame of `u` (u->resolution must be (w, h); u->part is ignored; params NULL = the defaults):
 *   (a) the first frame after create / reset: the G-buffer of u; the history is 0;
 *   (b) otherwise, if the pose of u (the bytes of resolution, mtr_sizes, focus, vec_to_mtr, top_drct, right_drct)
 *       differs from the previous frame's: the G-buffer of u, then image and history reprojected into the other pair
 *       of buffers, which becomes the current one; a resting camera pays for neither;
 *   (c) u with part = 1 into the sample frame through rt4_render_device_ex (d_counter counts as usual);
 *   (d) rt4_temporal_blend_device into the current image.
 * Asynchronous on `stream`: no allocation here, no synchronisation (the render's own buffers as rt4_render_device). A
 * resting camera's image equals the plain progressive run bit for bit. */
int rt4_temporal_frame_device(rt4_temporal* t, const rt4_uniforms* u, const rt4_reproject_params* params,
                              unsigned long long* d_counter, void* stream, char* err, size_t errlen);
/* Device pointers of the current image (`format`), its history and the G-buffer of the last frame's pose (so
 * rt4_denoise_device composes with them), each w x h with row stride w. They change with every frame call. */
void* rt4_temporal_image(const rt4_temporal* t);
int32_t* rt4_temporal_history(const rt4_temporal* t);
const rt4_gbuffer_px* rt4_temporal_gbuffer(const rt4_temporal* t);
/* The three copied to host buffers of w x h elements (any may be NULL). Synchronous: waits for the context's launches. */
int rt4_temporal_read_host(rt4_temporal* t, void* image, int32_t* history, rt4_gbuffer_px* gbuf, char* err, size_t errlen);
/* Device bytes the object owns. */
uint64_t rt4_temporal_bytes(const rt4_temporal* t);

/* ---- window-resolution output (the reference's sprite stretch, windows.cpp:25-33) ------------
 * The reference traces width / cell_size cells per row and stretches that texture over the window, so every cell
 * becomes a cell_size x cell_size block (RT4_UPSCALE_NEAREST). RT4_UPSCALE_GUIDED interpolates the cell colours
 * instead, for every window pixel only among the cells that lie on the pixel's own surface: the primary hit of a
 * window pixel (the G-buffer of the window's uniforms) is exact and cheap, so object edges come out at window
 * resolution. scale = cell_size; the window is W = cells_w*scale by H = cells_h*scale. G_cells is the G-buffer of
 * u_cells, G_win the G-buffer of u_window = rt4_upscale_uniforms(u_cells, scale).
 * Definition (fp32 round-to-nearest, no contraction, division and sqrt correctly rounded; dot is the fma chain of
 * DESIGN.md §3, mad(a,s,b) one fma per component; the kernel matches it bit for bit). For window pixel (x, y):
 * g = G_win(x, y), s = scale, cx = x / s, cy = y / s (integer division).
 *   1. NEAREST: the output pixel is the stored bits of cell (cx, cy), alpha included.
 *   2. GUIDED, the tap position (x shown, y alike): tx = 2*(x % s) + 1 - s; tx < 0: x0 = cx - 1, nx = tx + 2*s;
 *      otherwise x0 = cx, nx = tx; ax = (float)nx / (float)(2*s), one division (floor and frac of
 *      (x + 0.5)/s - 0.5 without rounding).
 *   3. X = mad(d, g.depth, focus), d the primary direction of (x, y) under u_window, op for op as
 *      rt4_render_gbuffer_device builds it; tol = plane_tol * fabsf(g.depth).
 *   4. Taps ty = 0,1 (outer), tx = 0,1 (inner): q = (x0+tx, y0+ty), k = (tx ? ax : 1-ax) * (ty ? ay : 1-ay). A tap
 *      counts iff q is inside the cell image, k > 0, G_cells(q).surface == g.surface and, when g.surface >= 0,
 *      dot(n_p, n_q) >= cos_min and fabsf(dot(n_p, X_q - X)) <= tol, where X_q = mad(d_q, z_q, focus), d_q the
 *      primary direction of cell q under u_cells and z_q = G_cells(q).depth. Comparisons with NaN are false: a hit
 *      with a non-finite depth has no counted tap. Two misses match with no further test (the sky interpolates among
 *      sky cells). A counted tap adds acc_c = acc_c + k * C(q)_c (a multiply, then an add; C decoded as in the
 *      filter) and wsum = wsum + k.
 *   5. wsum > 0: the colour acc / wsum in the frame's format (fma(c, 1, 0), then half: round to nearest even; RGBA8:
 *      the rule of rt4_frame_format) with alpha 1. Otherwise the stored bits of cell (cx, cy), as in NEAREST.
 * No reflectance threshold: a mirror's content is interpolated inside the mirror, only its outline is sharpened. */
enum rt4_upscale_mode { RT4_UPSCALE_NEAREST = 0, RT4_UPSCALE_GUIDED = 1 };
#define RT4_UPSCALE_MAX_SCALE 64
typedef struct rt4_upscale_params {
  int32_t mode;    /* rt4_upscale_mode */
  float cos_min;   /* smallest dot(n_p, n_q) a tap may have */
  float plane_tol; /* largest distance of the cell's hit point from the pixel's tangent plane, as a fraction of |depth| */
} rt4_upscale_params;
/* GUIDED, 0.9f, 0.02f. Starting points: nothing has been measured behind these values. */
void rt4_upscale_params_default(rt4_upscale_params* p);
/* *u_window = *u_cells with resolution multiplied by scale (exact integers in fp32); nothing else changes.
 * RT4_ERR_ARG for a NULL pointer, a scale outside 1..RT4_UPSCALE_MAX_SCALE, or a window wider than 65535 or taller
 * than 16383. */
int rt4_upscale_uniforms(const rt4_uniforms* u_cells, int32_t scale, rt4_uniforms* u_window);
/* d_cells: the cell frame (cells_w x cells_h, `format`); d_gcells: the G-buffer of u_cells; d_gwin: the G-buffer of
 * the window's uniforms (W x H); d_out: W x H in `format`. Strides in elements of their image. RT4_ERR_ARG, nothing
 * written, for a NULL pointer, an unknown format or mode, a scale outside 1..RT4_UPSCALE_MAX_SCALE, a resolution of
 * u_cells other than (cells_w, cells_h), a stride below its image's width, a misaligned pointer (G-buffers 16 B,
 * frames their pixel size) or an output that overlaps an input. NEAREST ignores, and accepts NULL for, both
 * G-buffers. Asynchronous on `stream`, no allocation. Ordered with the context's other launches. */
int rt4_upscale_device(rt4_context* ctx, const rt4_uniforms* u_cells, int32_t scale, const void* d_cells,
                       int64_t cells_stride, const rt4_gbuffer_px* d_gcells, int64_t gcells_stride,
                       const rt4_gbuffer_px* d_gwin, int64_t gwin_stride, void* d_out, int64_t out_stride, int32_t format,
                       int32_t cells_w, int32_t cells_h, const rt4_upscale_params* params, void* stream, char* err,
                       size_t errlen);
/* The same on host buffers (synchronous; output bytes outside the window keep their values). */
int rt4_upscale_host(rt4_context* ctx, const rt4_uniforms* u_cells, int32_t scale, const void* cells, int64_t cells_stride,
                     const rt4_gbuffer_px* gcells, int64_t gcells_stride, const rt4_gbuffer_px* gwin, int64_t gwin_stride,
                     void* out, int64_t out_stride, int32_t format, int32_t cells_w, int32_t cells_h,
                     const rt4_upscale_params* params, char* err, size_t errlen);

/* The state a frame loop needs to present cell frames at window resolution: the window image in `format`, the window
 * G-buffer, a cell G-buffer and the last present's uniforms, all allocated at creation (rt4_window_bytes). Destroy it
 * before its context. After rt4_context_set_scene call rt4_window_reset. */
typedef struct rt4_window rt4_window;
int rt4_window_create(rt4_context* ctx, int32_t cells_w, int32_t cells_h, int32_t scale, int32_t format, rt4_window** out,
                      char* err, size_t errlen);
void rt4_window_destroy(rt4_window* win); /* waits for the context's launches in flight */
/* The next present renders its G-buffers anew, as the first present after creation does. */
void rt4_window_reset(rt4_window* win);
/* Upscales the cell frame d_cells (cells_w x cells_h, `format`, stride in pixels) of the view u_cells into the window
 * image. GUIDED renders the window G-buffer, and the owned cell G-buffer when d_gcells is NULL, only when the pose of
 * u_cells (the bytes of resolution, mtr_sizes, focus, vec_to_mtr, top_drct, right_drct) differs from the last
 * present's or this is the first present after create / reset: a resting camera pays for the upscale alone. NEAREST
 * renders no G-buffer. d_gcells, when given, is the G-buffer of u_cells (rt4_temporal_gbuffer, or the one passed to
 * rt4_denoise_device). params NULL = the defaults. Asynchronous on `stream`: no allocation, no synchronisation. */
int rt4_window_present_device(rt4_window* win, const rt4_uniforms* u_cells, const void* d_cells, int64_t cells_stride,
                              const rt4_gbuffer_px* d_gcells, int64_t gcells_stride, const rt4_upscale_params* params,
                              void* stream, char* err, size_t errlen);
/* Device pointers of the window image (W x H, `format`, row stride W) and of the window G-buffer (row stride W). */
void* rt4_window_image(const rt4_window* win);
const rt4_gbuffer_px* rt4_window_gbuffer(const rt4_window* win);
/* The two copied to host buffers of W x H elements (either may be NULL). Synchronous: waits for the context's launches. */
int rt4_window_read_host(rt4_window* win, void* image, rt4_gbuffer_px* gbuf, char* err, size_t errlen);
/* Device bytes the object owns. */
uint64_t rt4_window_bytes(const rt4_window* win);

/* ---- light-domain accumulation with a per-pixel standard error (no reference counterpart) ----
 * Every other accumulator averages tone-mapped colours, as the reference's texture does. The tone curve
 * 1 - 1/(k*x + 1) is concave, so that average is darker than the image the samples describe, by an amount that
 * depends on how the samples are split into frames. This accumulator averages each frame's light (light sum /
 * samples) and tone-maps once, when the image is resolved; the running second moment of the luminance gives a
 * standard error per pixel for one more fma. Opt-in: the light average shows the fireflies that per-frame tone
 * mapping clamps, so the default accumulators do not change.
 * Definition (fp32 round-to-nearest, no contraction, division and sqrt correctly rounded, fma explicit; the kernels
 * match it bit for bit). One frame with light sum L (what the trace kernel hands the fold) for a pixel with state s:
 *   x_c = L_c / (float)samples (the division of the tone map); y = fma(0.2126f, x_r, fma(0.7152f, x_g, 0.0722f * x_b));
 *   n' = n + 1 (saturating at INT32_MAX); inv = 1.0f / (float)n';
 *   d_c = x_c - mean_c; mean_c' = fma(d_c, inv, mean_c);
 *   dy = y - mean_y; mean_y' = fma(dy, inv, mean_y); m2' = fma(dy, y - mean_y', m2).
 * Frames are applied in order. NaN and inf propagate as the operations give them (a NaN's payload is not defined).
 * Resolve: c = 1.0f - 1.0f / fma(k, mean_c, 1.0f) per channel, stored through the format's rule (the blend of
 * rt4_render_device_ex with part = 1 into a zero pixel: alpha 1); a pixel with n == 0 gets colour 0, alpha 1. After
 * exactly one frame mean = x, so the resolved RGBA32F image equals rt4_render_device_ex with part = 1 into zeros bit
 * for bit.
 * Noise, for a pixel with n >= 2: se = sqrtf((m2 / (float)(n - 1)) / (float)n), the standard error of mean_y;
 * t(v) = 1.0f - 1.0f / fma(k, v, 1.0f); q = t(mean_y + se) - t(mean_y): how far the displayed luminance moves when
 * the mean moves up one standard error, in display units. A pixel with n < 2 is unmeasured: se = q = +inf in the
 * maps, and it counts neither in `above` nor in the maxima.
 * The estimate is heavy-tailed: a pixel reads se = 0 until its first bright path arrives, so on scenes lit by small
 * emitters the share of pixels above a threshold RISES over the first hundred or so frames. It is an error map, not
 * a convergence test: do not stop a render because `above` is 0. */
typedef struct rt4_light_px { /* 32 B; all-zero bytes = the empty accumulator */
  float mean[3];     /* running mean of the frame's light, light sum / samples */
  float mean_y;      /* running mean of its luminance */
  float m2;          /* Welford sum of squared luminance deviations */
  int32_t n;         /* frames accumulated, saturating at INT32_MAX */
  float reserved[2]; /* written as 0 */
} rt4_light_px;

/* Exact (integer counts, maxima): the same for every order the tiles finish in. */
typedef struct rt4_noise_stats {
  uint64_t pixels, measured, above; /* w * h; pixels with n >= 2; measured pixels with q > threshold (false for NaN) */
  float max_q, max_se;              /* fmaxf over 0 and the measured pixels' values (NaN ignored); 0 when none */
} rt4_noise_stats;

/* rt4_render_frames_device into a light accumulator: n_frames frames of u[0], u[1], ... folded in order onto what
 * d_light holds (pixel (i, j) of the region at d_light + i*row_stride_px + j, as a frame; a banded region accumulates
 * its own pixels). A hipMemsetAsync to zero is the reset. u[f] may differ from u[0] only in seed and part, and part is
 * ignored. d_counter counts as usual. The frames run in launches of rt4_context_frames_per_launch frames through the
 * context's frame scratch (16 B per pixel and frame; a launch of one frame too): the first call with a larger scratch
 * need allocates (synchronises the stream once; rt4_context_reserve_frames does it ahead of time). RT4_ERR_ARG for a
 * region wider or taller than 8191 (the scratch's pixel word holds no more) and for a d_light that is not 16-byte
 * aligned. Asynchronous; ordered with the context's other launches. */
int rt4_render_light_device(rt4_context* ctx, const rt4_uniforms* u, int32_t n_frames, const rt4_region* region,
                            rt4_light_px* d_light, int64_t row_stride_px, unsigned long long* d_counter, void* stream,
                            char* err, size_t errlen);
/* The same onto a host accumulator (synchronous; bytes outside the region's pixels keep their values).
 * n_intersections (may be NULL) receives the count. */
int rt4_render_light_host(rt4_context* ctx, const rt4_uniforms* u, int32_t n_frames, const rt4_region* region,
                          rt4_light_px* light, int64_t row_stride_px, uint64_t* n_intersections, char* err, size_t errlen);
/* The w x h image of a light accumulator in `format`, tone-mapped with k. Strides in elements of their image.
 * RT4_ERR_ARG, nothing written, for a NULL pointer, an unknown format, w or h outside [1, 65535], a stride below w, a
 * misaligned pointer (accumulator 16 B, frame its pixel size) or a frame that overlaps the accumulator.
 * Asynchronous on `stream`, no allocation. Ordered with the context's other launches. */
int rt4_light_resolve_device(rt4_context* ctx, const rt4_light_px* d_light, int64_t light_stride, float k, void* d_frame,
                             int32_t format, int64_t frame_stride, int32_t w, int32_t h, void* stream, char* err,
                             size_t errlen);
int rt4_light_resolve_host(rt4_context* ctx, const rt4_light_px* light, int64_t light_stride, float k, void* frame,
                           int32_t format, int64_t frame_stride, int32_t w, int32_t h, char* err, size_t errlen);
/* The error maps and their statistics. d_se, d_q: float images (row stride map_stride floats); d_tile_above: int32,
 * `above` per 8x8 tile, row-major over ceil(w/8) x ceil(h/8) tiles, no padding; any of the three may be NULL. d_stats
 * (8-byte aligned) is written completely on every call: the call zeroes it on the stream first. RT4_ERR_ARG, nothing
 * written, for a NULL accumulator or d_stats, w or h outside [1, 65535], a stride below w, a misaligned pointer
 * (accumulator 16 B, maps and tiles 4 B, stats 8 B) or an output that overlaps the accumulator or another output.
 * Asynchronous on `stream`, no allocation. Ordered with the context's other launches. */
int rt4_light_noise_device(rt4_context* ctx, const rt4_light_px* d_light, int64_t light_stride, int32_t w, int32_t h,
                           float k, float threshold, float* d_se, float* d_q, int64_t map_stride, int32_t* d_tile_above,
                           rt4_noise_stats* d_stats, void* stream, char* err, size_t errlen);
int rt4_light_noise_host(rt4_context* ctx, const rt4_light_px* light, int64_t light_stride, int32_t w, int32_t h, float k,
                         float threshold, float* se, float* q, int64_t map_stride, int32_t* tile_above,
                         rt4_noise_stats* stats, char* err, size_t errlen);

/* ---- variance-guided a-trous filter of a light accumulator (no reference counterpart) ----
 * The filter of rt4_denoise_device run on the light means instead of on tone-mapped colours, with a luminance
 * edge-stop scaled by each pixel's own standard error, and tone-mapped once at the end (the SVGF scheme). Its support
 * shrinks as the standard error does, so it neither inherits the tone-map bias of a colour average nor goes on
 * blurring what varies inside one surface once the samples have resolved it. For display only: the accumulator is
 * read, never written. A and G (the G-buffer of the same view) share the pixel indexing [0,w) x [0,h).
 * Definition (fp32 round-to-nearest, no contraction, division and sqrt correctly rounded, fma explicit, dot the fma
 * chain of DESIGN.md §3; comparisons with NaN are false and a NaN's payload is not defined; the kernels match it bit
 * for bit):
 *   Level 0. p is filterable iff G.surface >= 0 && G.refl_prob <= max_refl_prob && A.n >= 2. id(p) = the surface of a
 *   filterable p, else -1. L_0 = A.mean, Y_0 = A.mean_y, V_0 = (A.m2 / (float)(n-1)) / (float)n (the radicand of se
 *   in rt4_light_noise_device).
 *   Level l = 0 .. levels-1, s = 2^l. A pixel that is not filterable keeps L, Y and V. For a filterable p:
 *   1. The variance pre-filter at unit stride, G3 = {1/4, 1/2, 1/4}: dy = -1..1 (outer), dx = -1..1 (inner),
 *      q = p + (dx, dy), g = G3[dy+1]*G3[dx+1]; a tap counts iff q == p, or q is inside the image and id(q) == id(p);
 *      for a counted tap va = va + g*V_l(q) (a multiply, then an add) and vw = vw + g.
 *      den = fma(sigma, sqrtf(va / vw), eps).
 *   2. The 25 taps: order, q = p + s*(dx, dy), H and k = H[dy+2]*H[dx+2] as in rt4_denoise_device. The centre tap has
 *      weight o = k. Any other tap passes the geometry test iff q is inside, id(q) == id(p), dot(n_p, n_q) >= cos_min
 *      and fabsf(z_q - z_p) <= depth_tol * z_p; for such a tap t = fabsf(Y_l(q) - Y_l(p)) / den,
 *      wl = 1.0f / fma(t, t, 1.0f), o = k * wl. A tap counts iff it is the centre, or it passes the geometry test and
 *      o > 0. For a counted tap: aL_c = aL_c + o*L_l(q)_c; aY = aY + o*Y_l(q); aV = aV + (o*o)*V_l(q) (the square,
 *      then the multiply, then the add); wsum = wsum + o.
 *   3. L_{l+1} = aL / wsum, Y_{l+1} = aY / wsum, V_{l+1} = aV / (wsum*wsum).
 *   The frame (any rt4_frame_format, alpha 1): a filterable pixel gets 1.0f - 1.0f / fma(k, L_levels_c, 1.0f) through
 *   the format's store rule; every other pixel gets exactly what rt4_light_resolve_device writes. So levels = 0, or a
 *   G-buffer of misses only, reproduces rt4_light_resolve_device byte for byte.
 *   d_filtered (float4 per pixel, may be NULL): a filterable pixel gets {L_r, L_g, L_b, V} of the last level, any
 *   other pixel {mean_r, mean_g, mean_b, n >= 2 ? V_0 : +inf}.
 * Mirrors (refl_prob above max_refl_prob), the sky and pixels with fewer than two frames pass through unfiltered.
 * With very few frames the variance estimate is poor (a pixel reads variance 0 until its first bright path arrives;
 * the pre-filter borrows the neighbours'): the filter still beats no filter, but a geometry-only filter does better
 * there. */
#define RT4_LIGHT_DENOISE_MAX_LEVELS 6
typedef struct rt4_light_denoise_params {
  int32_t levels;      /* 0 .. RT4_LIGHT_DENOISE_MAX_LEVELS; 0 = no filtering (the plain resolve) */
  float cos_min;       /* as rt4_denoise_params */
  float depth_tol;     /* as rt4_denoise_params */
  float max_refl_prob; /* as rt4_denoise_params */
  float sigma;         /* luminance tolerance in standard errors */
  float eps;           /* added to sigma * sd, in light units; >= 0 */
} rt4_light_denoise_params;
/* 5, 0.9f, 0.1f, 0.5f, 4.0f, 1e-6f: the values of the CPU prototype behind DESIGN.md §4.38's table (not tuned
 * further; sigma = +inf makes the filter geometry-only wherever the variance is positive). */
void rt4_light_denoise_params_default(rt4_light_denoise_params* p);
/* Strides in elements of their image (d_filtered: in float4). RT4_ERR_ARG, nothing written, for a NULL required
 * pointer, an unknown format, w or h outside [1, 65535], a stride below w, a misaligned pointer (accumulator, G-buffer
 * and d_filtered 16 B, frame its pixel size), levels outside [0, RT4_LIGHT_DENOISE_MAX_LEVELS], sigma or eps negative
 * or NaN, or an output that overlaps an input or the other output. Asynchronous on `stream`; ordered with the
 * context's other launches. The levels and the repacked guide live in context-owned scratch of their own
 * (rt4_context_light_denoise_bytes; rt4_context_denoise_bytes does not change): the first call that needs more waits
 * for the stream and allocates; rt4_context_destroy frees it. */
int rt4_light_denoise_device(rt4_context* ctx, const rt4_light_px* d_light, int64_t light_stride,
                             const rt4_gbuffer_px* d_gbuf, int64_t gbuf_stride, float k,
                             const rt4_light_denoise_params* params, void* d_frame, int32_t format, int64_t frame_stride,
                             float* d_filtered, int64_t filtered_stride, int32_t w, int32_t h, void* stream, char* err,
                             size_t errlen);
/* The same on host buffers (synchronous; bytes outside [0,w) x [0,h) keep their values). */
int rt4_light_denoise_host(rt4_context* ctx, const rt4_light_px* light, int64_t light_stride, const rt4_gbuffer_px* gbuf,
                           int64_t gbuf_stride, float k, const rt4_light_denoise_params* params, void* frame,
                           int32_t format, int64_t frame_stride, float* filtered, int64_t filtered_stride, int32_t w,
                           int32_t h, char* err, size_t errlen);
/* Bytes of the context's light-denoise scratch (0 before the first rt4_light_denoise_device call with levels > 0). */
uint64_t rt4_context_light_denoise_bytes(const rt4_context* ctx);

/* ---- adaptive light sampling: select noisy tiles, render only those (no reference counterpart) ----
 * The light accumulator keeps a frame count and a standard error per pixel; these two calls let a caller spend its
 * frames where that error is large. The policy (how many whole frames first, how often a whole frame again, when to
 * stop) stays with the caller: Tracer.render_light_adaptive (rt4.py) and rt4_render --light --adaptive run one.
 * Choosing samples from a pixel's own earlier samples is optional stopping: it biases the mean (DESIGN.md §4.39 has
 * the measured sizes). Dilation, the min_frames floor and periodic whole frames reduce the bias; none removes it.
 * Selection. Tiles are 8x8, numbered ty * tiles_x + tx with tiles_x = ceil(w/8): the numbering of d_tile_above. Only
 * pixels inside [0,w) x [0,h) count (never a padded row's padding).
 *   A pixel is hot iff n >= 2 && q > threshold, q op for op as in rt4_light_noise_device (false for a NaN q).
 *   A pixel is young iff n < min_frames.
 *   A tile qualifies iff it holds a young pixel or at least min_above hot pixels.
 *   A tile is selected iff some tile (tx+dx, ty+dy) inside the tile grid with |dx|, |dy| <= dilate qualifies (no
 *   wrap-around from the end of one tile row to the start of the next).
 * d_tiles[0 .. count) receives the selected tiles in ascending order (exact and deterministic); entries from count on
 * keep their bytes; d_tiles must hold tiles_x * tiles_y entries. *d_count receives count. d_tile_state (may be NULL;
 * tiles_x * tiles_y entries) receives 2 for a qualifying tile, 1 for a tile selected only by dilation, else 0. */
#define RT4_SELECT_MAX_DILATE 2
typedef struct rt4_tile_select_params {
  float threshold;    /* q threshold in display units, as rt4_light_noise_device; NaN is RT4_ERR_ARG */
  int32_t min_above;  /* 1..64: hot pixels a tile needs to qualify */
  int32_t min_frames; /* >= 0: a tile holding a pixel with n < min_frames qualifies whatever its noise */
  int32_t dilate;     /* 0..RT4_SELECT_MAX_DILATE: also take the tiles this close to a qualifying one */
} rt4_tile_select_params;
/* 1.0f / 255.0f (one 8-bit step), 4, 8, 1: the values of the CPU study behind DESIGN.md §4.39's table (not tuned further). */
void rt4_tile_select_params_default(rt4_tile_select_params* p);
/* RT4_ERR_ARG, nothing written, for a NULL pointer (d_tile_state excepted), w or h outside [1, 65535], a stride below w,
 * a misaligned pointer (accumulator 16 B, the others 4 B), a parameter outside its range, or an output that overlaps
 * the accumulator or another output. Asynchronous on `stream`; ordered with the context's other launches. The
 * per-tile flags live in context-owned scratch (rt4_context_select_bytes): the first call with more tiles than any
 * before waits for the stream and allocates; rt4_context_destroy frees it. */
int rt4_light_select_tiles_device(rt4_context* ctx, const rt4_light_px* d_light, int64_t light_stride, int32_t w, int32_t h,
                                  float k, const rt4_tile_select_params* params, uint32_t* d_tiles, uint32_t* d_count,
                                  int32_t* d_tile_state, void* stream, char* err, size_t errlen);
/* The same on host buffers (synchronous; tiles: tiles_x * tiles_y entries, those from *count on keep their bytes). */
int rt4_light_select_tiles_host(rt4_context* ctx, const rt4_light_px* light, int64_t light_stride, int32_t w, int32_t h,
                                float k, const rt4_tile_select_params* params, uint32_t* tiles, uint32_t* count,
                                int32_t* tile_state, char* err, size_t errlen);
/* rt4_render_light_device for the n_tiles listed tiles only. Tile numbers are region-local: ty * tiles_x + tx with
 * tiles_x = ceil(region.w/8), so for a whole-image region the numbering of selection; a banded or offset region
 * numbers its own rows. n_tiles is a host value (the caller reads *d_count back: one 4-byte read per pass). The
 * pixels of the listed tiles hold exactly the bytes rt4_render_light_device with the same u, n_frames and region
 * would have left in them; every other byte of d_light keeps its value; d_counter grows by the find_intersection calls
 * of the listed tiles' pixels only. n_tiles == 0 is RT4_OK and launches nothing. With tiles = tiles_x * tiles_y:
 * entries >= tiles are ignored; a tile listed twice leaves that tile's pixels unspecified (one or two applications of
 * each frame), never anything out of bounds. RT4_ERR_ARG for n_tiles < 0 or > tiles, a NULL or misaligned (4 B) list
 * with n_tiles > 0, and everything rt4_render_light_device refuses. The list is copied (clamped) into context-owned
 * scratch first, counted in rt4_context_select_bytes and sized for the region: the first call for a region with more
 * tiles than any before waits for the stream and allocates; after that the call neither synchronises nor allocates.
 * Asynchronous; ordered with the context's other launches. */
int rt4_render_light_tiles_device(rt4_context* ctx, const rt4_uniforms* u, int32_t n_frames, const rt4_region* region,
                                  const uint32_t* d_tiles, int32_t n_tiles, rt4_light_px* d_light, int64_t row_stride_px,
                                  unsigned long long* d_counter, void* stream, char* err, size_t errlen);
/* The same with a host list onto a host accumulator (synchronous). n_intersections (may be NULL) receives the count. */
int rt4_render_light_tiles_host(rt4_context* ctx, const rt4_uniforms* u, int32_t n_frames, const rt4_region* region,
                                const uint32_t* tiles, int32_t n_tiles, rt4_light_px* light, int64_t row_stride_px,
                                uint64_t* n_intersections, char* err, size_t errlen);
/* Bytes of the context's tile scratch: the selection's flags and the render's list copy (0 before the first call). */
uint64_t rt4_context_select_bytes(const rt4_context* ctx);

/* ---- light accumulators: merge, frame split, checkpoints (no reference counterpart) ----
 * Two light accumulators of the same view that hold disjoint sets of frames combine into the accumulator of all
 * their frames: Chan's pairwise update of the mean and the second moment. With it a render splits its frame numbers
 * over GPUs (every rank renders the whole image for its block of frames, the root merges), a checkpoint resumes, and
 * checkpoints of runs with other seeds pool.
 * Definition (fp32 round-to-nearest, no contraction, division correctly rounded, fma explicit; the kernel matches it
 * bit for bit; a NaN's payload is not defined; n >= 0 on both sides). State a (dst) and b (a source), per pixel:
 *   b.n == 0: a keeps the bits of its mean, mean_y, m2 and n.  Otherwise a.n == 0: a takes b's.  Otherwise:
 *   N = (int64)a.n + b.n; fb = (float)b.n / (float)N; wa = (float)a.n * fb;
 *   mean_c' = fma(b.mean_c - a.mean_c, fb, a.mean_c);
 *   dy = b.mean_y - a.mean_y; mean_y' = fma(dy, fb, a.mean_y);
 *   m2' = fma(dy * dy, wa, a.m2 + b.m2) (the product, the sum, then one fma);  n' = min(N, INT32_MAX).
 * reserved is written as 0 in all three cases. Empty operands are exact identities in either order, and m2 stays
 * >= 0 for m2 >= 0. Merging an accumulator of ONE frame into a gives the mean and mean_y of folding that frame
 * (rt4_render_light_device) bit for bit while N < INT32_MAX: fb is then 1 / (float)N, the fold's inv. It does NOT give
 * the fold's m2, which is fma(dy, y - mean_y', m2): the same number rounded differently. A merge of blocks is
 * therefore as accurate as one sequential fold (relative error against float64 within 1.25x of the
 * fold's), not bit-equal to it.
 * Source s, pixel (i, j) is d_srcs[s * src_plane_stride + i * src_stride + j]: the rank-major layout a gather leaves
 * on the root. The sources are applied as the left fold dst = merge(dst, src_0), then src_1, ...: one call with
 * n_srcs sources equals n_srcs calls with one source each bit for bit, and moves 32 (n_srcs + 2) B per pixel where
 * those move 96 n_srcs. RT4_ERR_ARG, nothing written, for a NULL pointer, n_srcs outside [1, RT4_LIGHT_MERGE_MAX],
 * w or h outside [1, 65535], a row stride below w, a plane stride below the span of one source image
 * ((h - 1) * src_stride + w; also with one source), a pointer not aligned to 16 B, or a dst that overlaps any source. Asynchronous on
 * `stream`, no allocation, no synchronisation. Ordered with the context's other launches. */
#define RT4_LIGHT_MERGE_MAX 16
int rt4_light_merge_device(rt4_context* ctx, rt4_light_px* d_dst, int64_t dst_stride, const rt4_light_px* d_srcs,
                           int64_t src_stride, int64_t src_plane_stride, int32_t n_srcs, int32_t w, int32_t h, void* stream,
                           char* err, size_t errlen);
/* The same on host accumulators (synchronous; the padding of dst keeps its bytes). */
int rt4_light_merge_host(rt4_context* ctx, rt4_light_px* dst, int64_t dst_stride, const rt4_light_px* srcs,
                         int64_t src_stride, int64_t src_plane_stride, int32_t n_srcs, int32_t w, int32_t h, char* err,
                         size_t errlen);
/* rt4_bands_unpermute_device for light accumulators: d_gathered holds world x rows_max rows of width rt4_light_px,
 * rank-major, d_image receives height rows of width pixels (row stride width). The same kernel in 16-B words and the
 * same checks; both pointers 16-byte aligned (RT4_ERR_ARG otherwise). Asynchronous on stream. */
int rt4_light_bands_unpermute_device(const rt4_light_px* d_gathered, rt4_light_px* d_image, int32_t width, int32_t height,
                                     int32_t world, int32_t band, int32_t rows_max, void* stream, char* err, size_t errlen);
/* The block of `rank` when n_frames frames are split over `world` ranks in contiguous blocks: count = n_frames / world
 * + (rank < n_frames % world), first = the frames of the ranks before it. The rank renders frames first + 1 ..
 * first + count of rt4_progressive_uniforms; with count == 0 it contributes an empty accumulator, which the merge
 * ignores (4d_ray_tracing_amd/shard.py frame_split is the same arithmetic). RT4_ERR_ARG for a NULL pointer,
 * n_frames < 0, world < 1 or rank outside [0, world). */
int rt4_frame_split(int32_t n_frames, int32_t world, int32_t rank, int32_t* first, int32_t* count, char* err,
                    size_t errlen);
/* Checkpoint of a light accumulator. File (little-endian): "RT4LIT1\0", int32 version (1), w, h, int64 frames_issued,
 * uint32 seed, uint32 key (rt4_accum_key of the run, 0 = not recorded), uint32 flags, uint32 0, then h rows of w
 * rt4_light_px, rows top first, no padding. frames_issued is the last frame number of rt4_progressive_uniforms that
 * was folded in: a resumed run continues with frames_issued + 1. It is a property of the run, not of any pixel: after
 * an adaptive run the pixels' n differ from it and from each other. RT4_LIGHT_POOLED marks a file that holds runs of
 * several seeds (seed and frames_issued are then those of the first run pooled) and cannot be resumed. A save writes
 * <path>.tmp, flushes it to the disk and renames it over path, as rt4_accum_save does. */
#define RT4_LIGHT_FILE_VERSION 1
#define RT4_LIGHT_POOLED 0x1u
int rt4_light_save(const char* path, const rt4_light_px* light, int32_t w, int32_t h, int64_t row_stride_px,
                   int64_t frames_issued, uint32_t seed, uint32_t key, uint32_t flags, char* err, size_t errlen);
/* Header only: any output pointer may be null. RT4_ERR_PARSE for a file that is not a light checkpoint (wrong magic or
 * version, a bad header) or whose size is not the header's plus w * h pixels. */
int rt4_light_info(const char* path, int32_t* w, int32_t* h, int64_t* frames_issued, uint32_t* seed, uint32_t* key,
                   uint32_t* flags, char* err, size_t errlen);
/* Reads the pixels into a host accumulator of the checkpoint's w and h (RT4_ERR_ARG if the caller's differ; bytes
 * outside the image keep their values); the header fields as rt4_light_info. Nothing is written for a file that is refused. */
int rt4_light_load(const char* path, rt4_light_px* light, int32_t w, int32_t h, int64_t row_stride_px,
                   int64_t* frames_issued, uint32_t* seed, uint32_t* key, uint32_t* flags, char* err, size_t errlen);

/* ---- supersampled light accumulators: s x s sub-pixel strata into one pixel (no reference counterpart) ----
 * Every sample of a pixel starts with the same primary ray (shader.frag:519-521), so a light accumulator converges to a
 * point-sampled picture: more frames remove noise, never the staircase on an outline. The view at s times the
 * resolution, rt4_upscale_uniforms(u, s), has its pixel centres on a regular s x s grid inside every pixel of u, and
 * rt4_render_light_device renders it into one accumulator per sub-pixel, each with its own random stream. This call
 * is the step back: the s x s sub-pixel accumulators (strata of equal area) into one accumulator per pixel that the
 * resolve, the noise map, the light filter, the tile selection and the checkpoints take unchanged. s^2 times fewer
 * frames at s times the resolution cast the same number of rays.
 * d_fine is (w*s) x (h*s), d_out is w x h. Definition (fp32 round-to-nearest, no contraction, division correctly
 * rounded; the kernel matches it bit for bit; a NaN's payload is not defined). For output pixel (X, Y) the strata are
 * i = b*s + a, the fine pixels (s*X + a, s*Y + b), b the outer loop and a the inner:
 *   inv = 1.0f / (float)(s*s); nmin = min_i n_i.
 *   nmin <= 0 (a stratum nobody sampled): the output pixel is 32 zero bytes, the empty accumulator. Otherwise:
 *   for each of mean_r, mean_g, mean_b, mean_y: sum = 0.0f; sum = sum + value_i in order; out = sum * inv.
 *   n' = nmin.
 *   nmin < 2: m2' = 0.0f. Otherwise:
 *     v_i = (m2_i / (float)(n_i - 1)) / (float)n_i (the radicand of se in rt4_light_noise_device, the same operations);
 *     sv = 0.0f; sv = sv + v_i in order; var = (sv * inv) * inv;
 *     m2' = (var * (float)nmin) * (float)(nmin - 1).
 *   reserved is written as 0.
 * The pixel's value is the equal-weight mean of s^2 independent strata, so its variance is the sum of the strata's
 * se^2 over s^4: var. m2' is chosen so that the consumers recover it: the downstream se =
 * sqrtf((m2' / (float)(n' - 1)) / (float)n') is sqrt(var) to within 1e-6 relative (four roundings on var, halved by
 * the root, plus the root's own), absent under- or overflow. Folding the strata as if they were frames of one variable
 * (rt4_light_merge_device) would count the differences BETWEEN strata, which are the image's detail, as noise: up to
 * 20 times too large an error on edges.
 * s = 1 runs the same formulas: mean, mean_y and n come out bit-equal to the input (0.0f + x and x * 1.0f are exact;
 * -0.0f comes out as +0.0f), m2 within those roundings.
 * Strata with different n (an adaptive run at the fine resolution) keep equal weights: the strata have equal area, and
 * weighting by n would bias towards whatever the selection favoured.
 * RT4_ERR_ARG, nothing written, for a NULL pointer, s outside [1, RT4_SUPERSAMPLE_MAX], w, h, w*s or h*s outside
 * [1, 65535], a stride below its image's width, a pointer not aligned to 16 B, or an output that overlaps the input.
 * Rendering bounds w*s and h*s further: rt4_render_light_device takes at most 8191 per side. Asynchronous on `stream`,
 * no allocation, no synchronisation. Ordered with the context's other launches. Memory-bound: 32 (s^2 + 1) B per
 * output pixel. */
#define RT4_SUPERSAMPLE_MAX 8
int rt4_light_downsample_device(rt4_context* ctx, const rt4_light_px* d_fine, int64_t fine_stride, rt4_light_px* d_out,
                                int64_t out_stride, int32_t w, int32_t h, int32_t s, void* stream, char* err,
                                size_t errlen);
/* The same on host accumulators (synchronous; the padding of out keeps its bytes; no alignment is asked of host
 * pointers). */
int rt4_light_downsample_host(rt4_context* ctx, const rt4_light_px* fine, int64_t fine_stride, rt4_light_px* out,
                              int64_t out_stride, int32_t w, int32_t h, int32_t s, char* err, size_t errlen);

/* ---- 3D retina view: the w-slices as a volume, projected (no reference counterpart) ----
 * An eye in 4D has a 3D retina: the matrix of rt4_uniforms (right_drct x top_drct) continued along the camera's fourth
 * axis, rt4_orientation.w_drct. The reference shows three orthogonal 2D sections through its centre; here the retina is
 * rendered whole, as `depth` slices, and projected to a picture that can be turned, so that the slices show parallax.
 * Once a volume is accumulated, a new view of it costs one projection and no tracing.
 * A volume of element type T holds voxel (s, i, j) at base + s*slice_stride + i*row_stride + j: j the column, i the row
 * (row 0 on top), s the slice; strides in elements, row_stride >= w, slice_stride >= (h-1)*row_stride + w.
 * Definition (fp32 round-to-nearest, no contraction, every fma explicit, division correctly rounded; comparisons with
 * NaN are false and a NaN's payload is not defined; the kernels match it bit for bit).
 *
 * 1. Slices (host only). Slice `slice` of `depth` is an ordinary render whose matrix centre is shifted along w_drct:
 *      t = (((float)slice + 0.5f) / (float)depth - 0.5f) * depth_size;
 *      out = *u; when t != 0: out.vec_to_mtr[c] = fmaf(w_drct[c], t, u->vec_to_mtr[c]);
 *      out.seed = (int32_t)((uint32_t)u->seed + (uint32_t)(slice - depth / 2) * 0x85EBCA6Bu)  (decorrelates the noise).
 *    depth_size is the retina's extent along w_drct at the matrix, in scene units (the natural choice: u->mtr_sizes[1]).
 *    The middle slice of an odd depth is *u byte for byte: the plain section.
 *
 * 2. Voxelize. L a light volume, G the G-buffer volume of the same slices (both w x h x d), k the tone-map constant.
 *      c_ch = (L.n == 0) ? 0 : 1.0f - 1.0f / fmaf(k, L.mean_ch, 1.0f)      (the resolve's formula);
 *      edge(v) iff G(v).surface >= 0 and one of v's six face neighbours that lie inside the volume has another surface
 *      value (-1, the sky, included);
 *      a = edge ? alpha_edge : (G(v).surface >= 0 ? alpha_fill : alpha_sky);
 *      V(v) = (a*c_r, a*c_g, a*c_b, a)                                        (plain multiplies: premultiplied).
 *    Why edges: in a 4D scene nearly every voxel hits something (the ground fills half the retina), and a volume of
 *    one opacity shows only its own faces. The sheets where the surface number changes are the objects' outlines.
 *
 * 3. Project. A view gives the picture's rays in voxel coordinates (x column, y row, z slice, voxel centres at the
 *    integers). For pixel (i, j) of the ow x oh picture (row 0 on top), c over x, y, z:
 *      a = ((float)j + 0.5f) / (float)ow - 0.5f;  b = 0.5f - ((float)i + 0.5f) / (float)oh;
 *      base_c = fmaf(b, dv_c, fmaf(a, du_c, origin_c));  sample n: f_c = fmaf((float)n + 0.5f, dt_c, base_c).
 *    A sample is outside unless f_c > -1.0f && f_c < (float)N_c on all three axes (N = w, h, d; tested before any
 *    conversion to an integer; NaN is outside). An outside sample contributes nothing. Otherwise x0 = floorf(f_x),
 *    wx1 = f_x - x0, wx0 = 1.0f - wx1, y and z alike; the eight taps run tz outer, ty, tx inner, tap (tx, ty, tz) is
 *    voxel (x0+tx, y0+ty, z0+tz) with weight (wz * wy) * wx; a tap whose index lies outside [0, N_c) on any axis is
 *    skipped; S_c = fmaf(weight, V_c, S_c) from 0, for r, g, b, a.
 *    Composite, from C = 0, T = 1, for n = 0 .. steps-1, inside samples only:
 *      C_c = fmaf(T, S_c, C_c);  T = T * fmaxf(1.0f - S_a, 0.0f);  then the ray stops if T < t_min.
 *    (fmaxf as IEEE maxNum: a NaN S_a gives 0.) The pixel is fmaf(T, background_c, C_c), alpha 1, stored through the
 *    format's rule (half: round to nearest even; RGBA8: the rule of rt4_frame_format).
 *    The kernel skips the samples ahead of and behind the volume in one step per ray; the bytes are those of the loop
 *    above (rt4_retina.h has the argument). */
#define RT4_RETINA_MAX_DEPTH 256
#define RT4_RETINA_MAX_STEPS 4096
/* RT4_ERR_ARG for a NULL pointer, depth outside 1..RT4_RETINA_MAX_DEPTH, slice outside [0, depth), or a depth_size that
 * is not finite and > 0. Host only. */
int rt4_retina_slice_uniforms(const rt4_uniforms* u, const float w_drct[4], int32_t depth, float depth_size,
                              int32_t slice, rt4_uniforms* out);

typedef struct rt4_retina_params {
  float alpha_sky, alpha_fill, alpha_edge; /* opacity of a voxel that misses / hits / hits next to another surface: [0, 1] */
  float t_min;                             /* a ray stops once its transmittance falls below this: [0, 1) */
  float background[3];                     /* what shows through, times the ray's last transmittance */
} rt4_retina_params;
/* 0, 1/32, 0.5, 1/256, black. Starting points, looked at on turntables of sphere, tiger and hypercube. */
void rt4_retina_params_default(rt4_retina_params* p);

typedef struct rt4_retina_view { /* the picture's rays in voxel coordinates: x column, y row, z slice, centres at integers */
  float origin[3], du[3], dv[3], dt[3];
  int32_t steps; /* samples per ray, 1..RT4_RETINA_MAX_STEPS */
} rt4_retina_view;
/* An orthographic view of the retina box (host only). The box is size[0] x size[1] x size[2] scene units (mtr_sizes[0],
 * mtr_sizes[1], depth_size) around the origin, X right, Y up, Z along the slices; scene to voxel per axis:
 * (X/Sx + 0.5)*w - 0.5, (0.5 - Y/Sy)*h - 0.5, (Z/Sz + 0.5)*d - 0.5. With yaw = pitch = 0 the rays run along +Z, slice 0
 * first. yaw turns about the retina's up axis: forward F = (sin yaw, 0, cos yaw), right R = (cos yaw, 0, -sin yaw);
 * then pitch about R: F' = cos(pitch) F - sin(pitch) Y (a positive pitch looks down on the box), U = cos(pitch) Y +
 * sin(pitch) F. The picture spans extent x extent*oh/ow scene units around the box centre (extent 0: the box diagonal):
 * du = R * extent, dv = U * extent*oh/ow. Every ray starts on the plane, normal to F', that touches the box in front
 * (e = (|F'x| Sx + |F'y| Sy + |F'z| Sz) / 2 before the centre's plane: at most half a diagonal) and runs 2e, to the
 * plane that touches it behind; the step is step_voxels times the smallest voxel edge min(Sx/w, Sy/h, Sz/d) and
 * steps = ceil(2e / step - 1/1024), at least 1 (an angle that is a right angle but for its float rounding adds no step).
 * Computed in double; each of the 12 floats is rounded once. RT4_ERR_ARG for a NULL pointer,
 * w, h, d, ow or oh < 1, a size, extent, angle or step_voxels that is not finite, a size or step_voxels <= 0, an
 * extent < 0, or more than RT4_RETINA_MAX_STEPS steps. */
int rt4_retina_view_make(int32_t w, int32_t h, int32_t d, const float size[3], float yaw, float pitch, float extent,
                         int32_t ow, int32_t oh, float step_voxels, rt4_retina_view* view, char* err, size_t errlen);

/* Step 2: d_voxels (float4 per voxel, 16-byte aligned) from d_light and d_gbuf, each with its own row and slice stride.
 * RT4_ERR_ARG, nothing written, for a NULL pointer, w or h outside [1, 65535], d outside 1..RT4_RETINA_MAX_DEPTH, a
 * stride too small, a pointer not aligned to 16 B, an alpha outside [0, 1], a t_min outside [0, 1) (a NaN fails both),
 * or a voxel volume that overlaps an input. Asynchronous on `stream`, no allocation. Ordered with the context's other
 * launches. */
int rt4_retina_voxelize_device(rt4_context* ctx, const rt4_light_px* d_light, int64_t light_row_stride,
                               int64_t light_slice_stride, const rt4_gbuffer_px* d_gbuf, int64_t gbuf_row_stride,
                               int64_t gbuf_slice_stride, float k, const rt4_retina_params* params, float* d_voxels,
                               int64_t vox_row_stride, int64_t vox_slice_stride, int32_t w, int32_t h, int32_t d,
                               void* stream, char* err, size_t errlen);
/* The same on host volumes (synchronous; the padding of the voxel volume keeps its bytes). */
int rt4_retina_voxelize_host(rt4_context* ctx, const rt4_light_px* light, int64_t light_row_stride,
                             int64_t light_slice_stride, const rt4_gbuffer_px* gbuf, int64_t gbuf_row_stride,
                             int64_t gbuf_slice_stride, float k, const rt4_retina_params* params, float* voxels,
                             int64_t vox_row_stride, int64_t vox_slice_stride, int32_t w, int32_t h, int32_t d, char* err,
                             size_t errlen);
/* Step 3: the ow x oh picture of `view` in `format` from a voxel volume; of params only t_min and background are used,
 * all are checked. Any finite view is accepted (rt4_retina_view_make need not have made it), and a view with NaN or
 * infinite numbers gives defined pixels too (the background wherever no sample is inside). RT4_ERR_ARG, nothing
 * written, for a NULL pointer, an unknown format, w or h outside [1, 65535], d outside 1..RT4_RETINA_MAX_DEPTH, ow or
 * oh outside [1, 65535], steps outside 1..RT4_RETINA_MAX_STEPS, a stride too small, a misaligned pointer (volume 16 B,
 * frame its pixel size), params as in voxelize, or a frame that overlaps the volume. Every load is index-checked,
 * offsets are 64-bit and the loop is bounded by steps. Asynchronous on `stream`, no allocation. Ordered with the
 * context's other launches. */
int rt4_retina_project_device(rt4_context* ctx, const float* d_voxels, int64_t vox_row_stride, int64_t vox_slice_stride,
                              int32_t w, int32_t h, int32_t d, const rt4_retina_view* view,
                              const rt4_retina_params* params, void* d_frame, int32_t format, int64_t frame_stride,
                              int32_t ow, int32_t oh, void* stream, char* err, size_t errlen);
/* The same on host buffers (synchronous; frame bytes outside [0,ow) x [0,oh) keep their values). */
int rt4_retina_project_host(rt4_context* ctx, const float* voxels, int64_t vox_row_stride, int64_t vox_slice_stride,
                            int32_t w, int32_t h, int32_t d, const rt4_retina_view* view, const rt4_retina_params* params,
                            void* frame, int32_t format, int64_t frame_stride, int32_t ow, int32_t oh, char* err,
                            size_t errlen);

/* The volume with its state: a light volume, a G-buffer volume and a voxel volume of w x h x depth (no padding: row
 * stride w, slice stride w*h), allocated at creation (rt4_retina_bytes), and what they were accumulated and voxelized
 * for. w, h in [1, 8191] (the light render's limit), depth 1..RT4_RETINA_MAX_DEPTH. A failed allocation returns
 * RT4_ERR_HIP with *out = NULL, which every call below accepts. Destroy it before its context. After
 * rt4_context_set_scene call rt4_retina_reset. */
typedef struct rt4_retina rt4_retina;
int rt4_retina_create(rt4_context* ctx, int32_t w, int32_t h, int32_t depth, rt4_retina** out, char* err, size_t errlen);
void rt4_retina_destroy(rt4_retina* ret); /* waits for the context's launches in flight */
/* The next accumulate starts over (frames_done 0), as the first after creation does. */
void rt4_retina_reset(rt4_retina* ret);
/* After create or reset, or when the bytes of u, w_drct or depth_size differ from the accumulated ones (then it resets
 * first): empties the light volume and renders the G-buffer volume, one rt4_render_gbuffer_device per slice. Then, for
 * every slice, folds frames frames_done + 1 .. frames_done + n_frames of rt4_progressive_uniforms of the slice's
 * uniforms (rt4_retina_slice_uniforms) into that slice's accumulator with rt4_render_light_device: every slice holds
 * exactly the bytes of those calls. u->resolution must be (w, h); n_frames >= 1; d_counter counts as usual.
 * One launch per slice and chunk of frames: a slice of a window-sized retina does not fill the GPU.
 * Asynchronous as rt4_render_light_device is. An error leaves the object reset. */
int rt4_retina_accumulate_device(rt4_retina* ret, const rt4_uniforms* u, const float w_drct[4], float depth_size,
                                 int32_t n_frames, unsigned long long* d_counter, void* stream, char* err, size_t errlen);
/* Voxelizes only when the volume was accumulated further, or the alphas or k differ, since the last voxelize; then
 * projects `view` into d_frame (ow x oh, `format`, stride in pixels). params NULL = the defaults. RT4_ERR_ARG before
 * the first accumulate. Asynchronous on `stream`: no allocation, no synchronisation. */
int rt4_retina_present_device(rt4_retina* ret, const rt4_retina_view* view, const rt4_retina_params* params, float k,
                              void* d_frame, int32_t format, int64_t frame_stride, int32_t ow, int32_t oh, void* stream,
                              char* err, size_t errlen);
/* Frames folded into every slice since the last reset. */
int64_t rt4_retina_frames_done(const rt4_retina* ret);
/* Device pointers of the three volumes. */
rt4_light_px* rt4_retina_light(const rt4_retina* ret);
rt4_gbuffer_px* rt4_retina_gbuffer(const rt4_retina* ret);
float* rt4_retina_voxels(const rt4_retina* ret);
/* The three copied to host volumes of w x h x depth elements (any may be NULL). Synchronous: waits for the context's
 * launches. */
int rt4_retina_read_host(rt4_retina* ret, rt4_light_px* light, rt4_gbuffer_px* gbuf, float* voxels, char* err,
                         size_t errlen);
/* Device bytes the object owns. */
uint64_t rt4_retina_bytes(const rt4_retina* ret);

/* ---- diagnostics (used by the parity tests; not on the render path) ------------------------- */
/* Bytes of the context's frame-colour scratch for pipelined frames (0 before any pipelined launch or
 * reservation; a scene that runs frame by frame never allocates it). */
uint64_t rt4_context_frame_scratch_bytes(const rt4_context* ctx);
/* Bytes of the context's overlap slot buffers (without RT4_FLAG_SERIAL_FRAMES, the default: 0 before any single-frame
 * launch or reservation; a context made with RT4_FLAG_SERIAL_FRAMES always returns 0). */
uint64_t rt4_context_overlap_bytes(const rt4_context* ctx);
/* Allocates the slot buffers that overlapped single-frame launches of one w x h image use with the context's
 * current scene (3, or 8 for a frame too small to fill the chip), so that the first such launch neither
 * allocates nor synchronises. Waits for the context's launches in flight when it grows a buffer. A no-op for a
 * context made with RT4_FLAG_SERIAL_FRAMES. For the 4D view's sections pass w x h with w * h >= the sections'
 * pixels together. */
int rt4_context_reserve_overlap(rt4_context* ctx, int32_t w, int32_t h, char* err, size_t errlen);
enum rt4_eval_fn {
  RT4_EVAL_ACOS = 0, RT4_EVAL_ASIN = 1, RT4_EVAL_SIN = 2, RT4_EVAL_COS = 3,
  RT4_EVAL_VOLUME_BY_W = 4, /* shader.frag:136-138 */
  RT4_EVAL_W_BY_VOLUME = 5, /* shader.frag:141-150; aux[i] = Newton iterations */
  RT4_EVAL_HASH = 6,        /* shader.frag:94-102 on the bit pattern of in[i] */
  RT4_EVAL_SQRT = 7         /* the kernel's correctly rounded sqrt (GLSL sqrt, e.g. :47, :137, :216) */
};
/* Evaluates a device math function element-wise (synchronous; host buffers). */
int rt4_debug_eval(rt4_context* ctx, int fn, const float* in, float* out, int32_t* aux, int64_t n, char* err,
                   size_t errlen);

/* Runs find_intersection (shader.frag:434-451) for n rays of the context's scene on the device.
 * rays: n x 8 floats (point xyzw, drct xyzw). out: n x 8 floats {hit(0/1), dist, norm xyzw,
 * glow, refl_prob}; out_color: n x 3 floats. Synchronous; host buffers. */
int rt4_debug_find_intersection(rt4_context* ctx, const float* rays, float* out, float* out_color, int64_t n,
                                char* err, size_t errlen);

/* Runs the trace kernels' final_light (shader.frag:454-468 behind the sky shortcuts of the context's scene) for n
 * escaping directions, one lane each. drct: n x 4 floats, as they are (not normalised); out: n x 3 floats.
 * Synchronous; host buffers. RT4_ERR_ARG (nothing written) for a NULL pointer, n < 0 or a context without a scene. */
int rt4_debug_final_light(rt4_context* ctx, const float* drct, float* out, int64_t n, char* err, size_t errlen);

/* The trace kernels' bounding-ball decisions (their own device functions, on the context's scene) for n rays, one
 * lane each. rays: n x 8 floats (point xyzw, drct xyzw), as they are. out_mask: one uint32 per ray:
 *   bit 0      the exact test of union 0 is skipped (the ray's line clears its ball, or the ball lies behind),
 *   bit 1      the same for tiger 0,
 *   bit 2      the ray's line clears hypercube 0's ball (its faces skip the exact test unless nearly parallel),
 *   bits 8-15  the cells of hypercube 0 that the cull pass rejected (bit 8 + k: cell k).
 * A figure that the scene lacks gives 0 in its bits; so does a ball the host disabled. The skips belong to the
 * specialised kernels (the generic find_intersection tests everything); the mask is the same under either flag.
 * Synchronous; host buffers. RT4_ERR_ARG (nothing written) for a NULL pointer, n < 0 or a context without a scene. */
int rt4_debug_bound_skip(rt4_context* ctx, const float* rays, uint32_t* out_mask, int64_t n, char* err, size_t errlen);

/* The trace kernels' sphere-cull decisions (their own device functions, on the context's scene and its constants) for
 * n rays, one lane each. rays: n x 8 floats (point xyzw, drct xyzw), as they are. out: two uint32 per ray:
 *   word 0, bit i           sphere i is not pending after the cull pass: its exact test is skipped (the ray starts
 *                           outside and points away, or its line clears the sphere by the cull's margin),
 *   word 1, bit i (i < 16)  cylinder i's exact part is skipped by the same cull on the projected ray (0 for a ray
 *                           whose projection onto the cylinder's plane misses before the cull is asked),
 *   word 1, bit 16 + 2u + c the same for cylinder c (0 / 1) of union u.
 * An object that the scene lacks gives 0; so does a cull the host disabled, but for the spheres' early-out of rays
 * that point away, which needs none of the host's margin. The mask is the same under either kernel flag.
 * Synchronous; host buffers. RT4_ERR_ARG (nothing written) for a NULL pointer, n < 0 or a context without a scene. */
int rt4_debug_cull(rt4_context* ctx, const float* rays, uint32_t* out, int64_t n, char* err, size_t errlen);

/* The thresholds rt4_context_set_scene makes from a radius r for the band filters of the union and the tiger, which
 * compare the squared distance q to the other axes pair without a square root: for every float q that dot(v, v) can
 * give (+0, denormals, normals, +inf, NaN)
 *   q > *gt  <=>  sqrt(q) > r      and      q < *lt  <=>  sqrt(q) < r      (sqrt correctly rounded).
 * *gt is +inf for a NaN or infinite r and negative for a negative one; *lt is 0 for a NaN, zero or negative r.
 * Host only: no context, no device. RT4_ERR_ARG for a NULL pointer. */
int rt4_debug_sqrt_thresholds(float r, float* gt, float* lt);

/* Counts the 32-bit patterns x for which the kernel's sqrt (fast path without input scaling) differs
 * from the IEEE square root; 0 expected. Exhaustive over all 2^32 inputs on the device (~10 ms). */
int rt4_debug_verify_sqrt(rt4_context* ctx, uint64_t* mismatches, char* err, size_t errlen);

/* find_intersection calls the context's launches actually evaluated since the last reset (all of them
 * unless RT4_FLAG_PRIMARY_REUSE: only its launches count). Waits for the context's last launch. */
int rt4_context_evaluated(rt4_context* ctx, uint64_t* n, int32_t reset, char* err, size_t errlen);

/* The scene-constant checks of rt4_context_set_scene, alone (synchronous). verify_div: mismatches of
 * the verified-divisor quotient against x / b over the reduced sweep (full = 0: positive numerators,
 * edge exponents + three of the middle band) or over all 2^32 numerators (full = 1);
 * set_scene enables the fast quotient iff the reduced count is 0. sky_threshold: the smallest float c
 * with acos(c) < ang in the kernel's acos (NaN: none), over c in (0.5, 1] for ang <= 1 (full = 0) or
 * over all 2^32 patterns (full = 1). */
int rt4_debug_verify_div(rt4_context* ctx, float b, int32_t full, uint64_t* mismatches, char* err, size_t errlen);
int rt4_debug_sky_threshold(rt4_context* ctx, float ang, int32_t full, float* c_min, char* err, size_t errlen);

/* Trace kernel selected for the context's scene: 0xFFFFFFFF = the generic find_intersection
 * (any group list); otherwise the K_* group bits (low byte: 1 spaces, 2 spheres, 4 cylinders,
 * 8 union, 16 hypercube, 32 tiger), plus (n_spaces+1) << 8 | (n_spheres+1) << 16 |
 * (n_cylinders+1) << 24 when a kernel compiled for the scene's exact object counts exists.
 * 0 if the context has no scene. */
uint32_t rt4_context_kernel_shape(const rt4_context* ctx);

#ifdef __cplusplus
}
#endif

#endif /* RT4_H */
