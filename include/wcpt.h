/*
 * wcpt.h — C-ABI drop-in boundary for the WC-Path-tracer compute path on MI355X (gfx950).
 *
 * This header is the only interface the reference's Jai host would see. It replaces the
 * Vulkan compute dispatch of `src/PathTracingRenderer.jai` (reference @ /root/reference):
 *
 *   reference (file:line)                                   replaced by
 *   -----------------------------------------------------   -----------------------------------------
 *   DBufferManager Allocate   src/BufferManager.jai:19-34    wcpt_buffer_alloc
 *   DBufferManager Update     src/BufferManager.jai:52-64    wcpt_buffer_upload   (grow-on-demand, :53-54)
 *   DBufferManager Free       src/BufferManager.jai:36-45    wcpt_buffer_free
 *   GetDeviceAddress          modules/VKUtils/Buffer.jai:101  wcpt_buffer_device_address
 *   CreateScreen              src/PathTracingRenderer.jai:345 wcpt_create_screen  (rgba32f image -> float4[H][W])
 *   Resize                    src/PathTracingRenderer.jai:393 wcpt_resize
 *   Render (push block + vkCmdDispatch)
 *                             src/PathTracingRenderer.jai:399-457  wcpt_render (SceneData by value + 3 BDAs)
 *   Submit / timeline wait    modules/VKUtils/Synchronization.jai:64-89, src/main.jai:73-95  wcpt_sync
 *   Deinit                    src/PathTracingRenderer.jai:473 wcpt_destroy
 *
 * Byte layouts of the POD types are the reference's GLSL `scalar` block layouts, which are identical to
 * the Jai structs (src/shaders/pathTracer.comp:10-95, src/PathTracingRenderer.jai:38-140).
 *
 * Errors: every entry point returns int (0 = success, negative = error; -1..-13 keep VkResult meaning).
 * Nothing aborts or exits. wcpt_last_error() gives a human-readable message.
 * Threading: one context per device; calls on one context are not thread-safe (the reference drives the
 * renderer from a single thread, src/main.jai:185-194).
 */
#ifndef WCPT_H
#define WCPT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: wcpt_counters gained ref_stack_overflow_segments / ref_stack_max; the wcpt_group_* multi-device entry points.
 * 3: groups overlap each frame's gather with the next frame's render; wcpt_group_create_ex (transports),
 *    wcpt_group_unique_id / wcpt_group_create_rank (one process per device), wcpt_group_set_option, wcpt_group_info.
 * 4: WCPT_GROUP_OPTION_THREADS (each local rank's share of a frame issued from a host thread of its own);
 *    wcpt_group_info gained issue_threads; wcpt_group_set_output reads `bytes` in every process. Later additions that
 *    keep the layouts and calls (no version step): WCPT_GROUP_TRANSPORT_DIRECT, WCPT_OPTION_PROFILE_REGION,
 *    WCPT_OPTION_WF_FETCH, WCPT_OPTION_WF_PIPES 0 (automatic, now the default), wcpt_bvh_refit,
 *    wcpt_bvh_refit_device, wcpt_wf_last_plan, wcpt_trace_primary, wcpt_pick. */
#define WCPT_ABI_VERSION 4

/* ---- error codes (VkResult-compatible where a VkResult exists) ---------------------------------- */
#define WCPT_SUCCESS                      0
#define WCPT_ERROR_OUT_OF_HOST_MEMORY    (-1)
#define WCPT_ERROR_OUT_OF_DEVICE_MEMORY  (-2)
#define WCPT_ERROR_INITIALIZATION_FAILED (-3)
#define WCPT_ERROR_DEVICE_LOST           (-4)
#define WCPT_ERROR_UNKNOWN               (-13)
#define WCPT_ERROR_INVALID_ARGUMENT      (-1000)
#define WCPT_ERROR_INVALID_HANDLE        (-1001)
/* A far child did not fit the 48-entry traversal stack: the push is refused, nothing is written past
 * the stack, and that subtree is not visited. wcpt_render itself returns success; the next wcpt_sync or wcpt_readback
 * reports the error once and clears it. wcpt_render_counters on such a tree returns it too, and the counters it wrote
 * are those of the cut-short traversal, not the reference's. */
#define WCPT_ERROR_STACK_OVERFLOW        (-1002)
#define WCPT_ERROR_NO_SCREEN             (-1003) /* wcpt_render before wcpt_create_screen */
#define WCPT_ERROR_PARSE                 (-1004) /* OBJ text could not be parsed */

/* ---- material types (pathTracer.comp:30-33, PathTracingRenderer.jai:53-56) ---------------------- */
#define WCPT_MATERIAL_METAL      0u
#define WCPT_MATERIAL_DIELECTRIC 1u

/* ---- kernel variants ---------------------------------------------------------------------------- */
#define WCPT_KERNEL_MEGAKERNEL  0  /* one lane per pixel, exact reference semantics (default)          */
#define WCPT_KERNEL_WAVEFRONT   2  /* split ray-gen / traverse / shade queues (same semantics)         */
/* Chosen per render from the scene: the megakernel where the draws' leaves hold several triangles each (the pair-record
 * layout: Cornell-class and the reference's mushroom), the wavefront kernel for thin-leaf meshes (a Sponza-scale
 * midpoint BVH, ~2 triangles per leaf), the faster of the two on every bench scene. Same results either way. */
#define WCPT_KERNEL_AUTO        1

/* ---- tuning options (wcpt_set_option); none changes results ------------------------------------- */
#define WCPT_OPTION_STACK       1  /* megakernel traversal stack: 0 = scratch, 1 = LDS + spill (default) */
#define WCPT_OPTION_DIAGNOSTICS 2  /* 1: wcpt_render_counters also fills the SIMD-efficiency fields      */
#define WCPT_OPTION_SORT_RAYS   3  /* wavefront: sort bounce rays by (octant, origin Morton) (default 0) */
#define WCPT_OPTION_WF_STACK    4  /* wavefront: LDS traversal-stack entries per lane, 10 | 16 | 24 (default 10) */
/* Derived triangle records. wcpt_render derives per draw command one 48-byte record per triangle (a, b-a, c-a)
 * from the draw's index and vertex buffers; leaf tests read them instead of index + vertex gathers (same
 * arithmetic, same results). 1 (default): rebuilt only when a draw's buffers were re-uploaded through
 * wcpt_buffer_upload / re-allocated, or its buffers or index count changed; the draw commands themselves are read
 * from the context's host copy of what wcpt_buffer_upload wrote (bytes never uploaded are read from the device).
 * The same cache holds what the runtime learns about each draw's BVH buffer (whether every leaf is small and lies on
 * the derived records, which selects the wavefront's fast leaf layout); it is re-learned when the BVH buffer is
 * re-uploaded through wcpt_buffer_upload or re-allocated.
 * 0: the draw commands are read from the device, the records rebuilt on every render and the fast leaf layout is not
 * used (use this when the application writes draw-command, vertex, index or BVH buffers by other means, e.g. hipMemcpy
 * to a wcpt_buffer_device_address, a refit or its own kernels: with 1, such writes into uploaded ranges are not
 * seen). A BVH rewritten behind the cache can give a wrong image but never a read outside the derived records.
 * Vertex or index buffers the context does not know (addresses that are no wcpt_buffer of this context): with 1 their
 * records are never kept from one frame preparation to the next, but a render that reuses the preparation of the render
 * before -- draw commands uploaded to this context, and no wcpt_buffer_alloc / _upload / _free or option change on it
 * since -- renders the records of that render, so writes into such buffers are not seen until one of those calls; with
 * draw commands the context reads from the device every render prepares anew.
 * The library's own refit is the exception: wcpt_bvh_refit_device counts as a write of the node AND the vertex buffer,
 * so vertices written by other means followed by that call are seen with the option left at 1. */
#define WCPT_OPTION_TRIANGLE_CACHE 5
/* Megakernel leaf tests: -1 (default) choose by mean triangles per leaf; 0 single records; 1 pair records
 * (two triangles per lane with packed-FP32 arithmetic). Results are identical either way. */
#define WCPT_OPTION_PAIR_RECORDS 6
/* Traversal stack entries carry the deferred child's (left, count) (1, default, when the draw's BVH buffer is a
 * context buffer of < 2^24 nodes) so a pop needs no node fetch; 0: entries hold node indices. Same results. */
#define WCPT_OPTION_PACKED_REFS 7
/* Wavefront trace: a wave fetches new rays once this many of its 64 lanes are idle (1..64, default 20: fewer,
 * fuller fetch rounds; c3 9.0 -> 8.2 ms at 12 against 1; round 5, with the finished lanes' hit records stored at the
 * refill: c4 197.8-198.2 ms at 20 against 199.5 at 12 and 201.3 at 32, c3 unchanged within the spread). The
 * path-persistent trace (WCPT_OPTION_WF_PERSIST) reads it as its fetch and shading-batch threshold too, with its own
 * default of 12 while the option is unset (round 6: c3 8-way shares 1 % faster than at 20); a value set here governs
 * both. */
#define WCPT_OPTION_WF_REFILL 8
/* Megakernel tile order: 0 each XCD walks a contiguous band of 8x8 tiles; 1 scattered (tile b * m mod tiles), so the
 * tiles resident on a CU at once come from all over the frame; 3, 4, 5, 6 XCD bands striped by 1, 2, 4, 8 tile rows
 * (XCD x walks the stripes s = x mod 8, so every XCD sees every part of the frame while neighbouring tiles stay
 * together); 2 (default) cost-ordered: every render records each tile's time, and after the first render of a frame
 * geometry (width, rows, first row) and every 64 renders the tiles are sorted by it, longest first, for the renders
 * that follow (the launch's last round then holds the short tiles). Until the first sort: scattered when the launch
 * fits in about one round of resident waves, stripes of one tile row otherwise. Same results in every order. */
#define WCPT_OPTION_MK_TILE_ORDER 9
/* Wavefront: concurrent pipelines (1..4, or 0 = the default: on the path-persistent trace 1, or 2 under the frame
 * overlap; else 3 when the frame holds at most 8 paths per resident trace lane, else 2). Pipeline j renders the 8x8
 * tiles t with t % K == j on its own stream, so one pipeline's trace tail (a few slow rays) overlaps another's bulk.
 * Same results. */
#define WCPT_OPTION_WF_PIPES 10
/* Kernel timing (wcpt_profile_begin / wcpt_profile_end): 0 (default) one pair of HIP events around every render;
 * 1 two events for the whole profiled region, one before its first render and one recorded by wcpt_profile_end, so
 * kernel_ms_total spans the renders' launches and the gaps between them, and launches counts the renders. Each event
 * record is a packet on the stream: per-render pairs cost ~1.3 % of a 0.36-ms frame (c2: 0.3651-0.3660 against
 * 0.3607-0.3611 ms per frame without, profiles/r05_events_ab.log). Set it outside a profiled region. With 1 a
 * wcpt_trace_primary pass counts like a render (with 0 it is not timed). */
#define WCPT_OPTION_PROFILE_REGION 11
/* Wavefront trace: fetch rounds per traversal iteration. 1: the child pair of an interior lane and the triangle of a
 * leaf lane are fetched together (a lane that descends into a leaf tests it the next iteration); 0: the leaf fetch
 * follows the interior step, so a descent tests its first triangle in the same iteration; -1 (default): one round
 * when a pipeline's queue holds at most 8 rays per resident trace lane (fetch latency exposed), two otherwise
 * (issue-bound). Same results. */
#define WCPT_OPTION_WF_FETCH 12
/* Wavefront: the path-persistent trace, one launch per frame in which each lane runs its path's segments one after
 * another and shades between them, for one sample per pixel on one-draw scenes. -1 (default): where the frame has at
 * most 1.4 paths per resident lane of it (row blocks), 0 never, 1 whenever eligible. Same results. */
#define WCPT_OPTION_WF_PERSIST 13
/* The gather output (wcpt_set_gather_output) addressed by frame row: 1 = the pixel of frame row y goes to row y of
 * the output (a buffer of the whole frame, which several contexts can share, each writing only its own rows -- rows
 * blocks or interleaved stripes alike); 0 (default) = the context's rows back to back (row ly of its rows at row ly).
 * Added under ABI 4. */
#define WCPT_OPTION_GATHER_FRAME_ROWS 14
/* Frame overlap (megakernel, cost-ordered tiles): consecutive renders with no other call on the context between them
 * run as two pipes, each on a stream of its own and owning half the tiles (the same pixels in every frame), so one
 * pipe's next frame starts in the other's last round of waves instead of behind the whole frame. Every other entry
 * point (wcpt_sync, readback, composite, profile end, buffer calls, a group's exchange ...) first orders the context's
 * stream after both pipes, so what it sees or queues is as if each render had run on the stream; hence only on the
 * context's own stream (not after wcpt_set_stream) and not under per-render timing events. 1 (default): megakernel
 * launches from 1.5 rounds of resident waves up (a 1920x1080 frame or its 2- and 4-way row blocks, not an 8-way block),
 * wavefront frames of several pipelines; 0 off; 2 whenever the tiles are cost-ordered (worth it on a one-round launch
 * whose waves differ much in length: the reference's scene in an 8-way block 0.308 -> 0.260 ms, the Cornell box +0.9 %).
 * Same results. Added under ABI 4. */
#define WCPT_OPTION_FRAME_OVERLAP 15
/* Primary cache (megakernel). The primary ray of a pixel depends only on the pixel, the frame size, inverseProjection,
 * inverseView and position -- no random number -- so while the camera and the scene stand still every progressive frame
 * finds the primary segment of the frame before. 1 (default): the first render after frame 0 of such a sequence stores
 * each pixel's resolved primary segment -- the ray's direction, the hit's distance, facing, normal and material index:
 * 32 bytes per pixel of the context's rows, whatever the number of draw commands (66 MB for 1920 x 1080), allocated
 * when a render first writes -- and the renders that follow read it instead of computing the direction, tracing the
 * primary segment and resolving its hit; shading runs as ever, from the current material buffer. A render with
 * renderedFramesCount == 0 drops the cache and renders plainly, so a camera that
 * moves every frame pays nothing. The cache is also dropped when anything the record depends on changes: the camera's
 * bytes, sphereCount, drawCommandCount, the frame size or the context's rows, the sphere or draw-command address, any
 * wcpt_buffer_alloc / wcpt_buffer_upload / wcpt_buffer_free, an option change, or a render by the wavefront kernel.
 * wcpt_render_counters never uses it. 0: off. It is active only while WCPT_OPTION_TRIANGLE_CACHE is 1, and it relies
 * on the same promise, now extended to the sphere buffer: scene buffers change through wcpt_buffer_upload, or the
 * application resets renderedFramesCount to 0 (as the reference's editor does whenever something moves).
 * Same results. Added under ABI 4. */
#define WCPT_OPTION_PRIMARY_CACHE 16
/* Split renders (megakernel). A wave keeps issuing a segment's traversal while any of its 64 paths is alive, and in an
 * open scene paths end bounce by bounce. k >= 1: a one-sample render on the LDS stack runs as two launches on the same
 * stream -- the kernel up to segment k (segments count from 0, the primary one), whose surviving paths go to a queue of
 * 56 bytes per pixel of the context's rows (allocated when a render first splits), and a launch that finishes them one
 * per lane in full waves. k > maxBounceCount, samples > 1 and WCPT_OPTION_STACK 0 render in one launch. 0: never. -1
 * (default): automatic -- before segment 3 (or maxBounceCount, if less) for renders of 3 rounds of resident waves or
 * more with maxBounceCount >= 2 (a 1920x1080 frame or its halves, not its 4- or 8-way blocks) of a scene with at most
 * 64 triangles: the second launch's waves hold paths of unrelated tiles, which costs a larger mesh more than the
 * fuller waves save (the Cornell box -3.7 %, the reference's scene +6 % when forced; csrc/mk_split_rule.h has the
 * measurements). Values outside -1..15 are refused. Same results.
 * Added under ABI 4. */
#define WCPT_OPTION_MK_SPLIT 18
/* Tiny trees (megakernel split renders, exact arithmetic, pair records, one draw command). A draw whose BVH is a
 * root leaf, or a root over two leaves -- what the reference's builder makes of a mesh of a few dozen triangles or
 * fewer -- is walked without the traversal loop: the wave reads the nodes through the scalar cache and tests the
 * leaves in the reference's order, with the reference's box tests and culls per lane (csrc/mk_tiny_rule.h has the
 * rule). A wave whose lanes disagree on the children's order tests the leaves in both orders, each for its own
 * lanes. -1 (default): automatic -- wherever the rule allows; 0: never; 1: wherever the rule allows. The walk has
 * kernels of its own, which take the places of the two launches of a split render (WCPT_OPTION_MK_SPLIT: by itself
 * the large one-sample frames of scenes of at most 64 triangles, or a forced cut), so a render in one launch -- a
 * small frame, samples > 1, every larger mesh -- runs the kernel it ran before. Further only where the draw takes pair records
 * (WCPT_OPTION_PAIR_RECORDS: by itself from 4 triangles per leaf up, so the Cornell room does and a mesh of a few
 * triangles does not unless the option is 1), only in WCPT_ARITH_EXACT (the fast-arithmetic kernels keep the loop)
 * and only while WCPT_OPTION_TRIANGLE_CACHE is 1 (the tree is classified once per BVH buffer generation). Values
 * outside -1..1 are refused. Same results. Added under ABI 4. */
#define WCPT_OPTION_MK_TINY_TREE 19

/* ---- options that change results (wcpt_set_option) ---------------------------------------------------------- */
/* Arithmetic of the megakernel's render launches. WCPT_ARITH_EXACT (0, default): the reference's operand order, unfused,
 * with correctly rounded reciprocal and square root and the deterministic software log / cos -- bit-identical to the
 * CPU oracle. WCPT_ARITH_FAST (1) is a permission for a host that renders for display: megakernel render launches then
 * take the fast instances, which relax
 *   - the dot and cross products of the triangle tests and of the shading arithmetic (reflect, refract, the Fresnel
 *     term, normalize, p + t * d) to fused multiply-adds, written out in the source -- the library is still built
 *     without floating-point contraction, so which products fuse is defined, not chosen by the compiler. The sphere
 *     test keeps its unfused products (its discriminant is cancellation-dominated on a large sphere, and fusing it
 *     tripled the diverged pixels of the reference's scene) and takes only the hardware sqrt;
 *   - 1/x and vector / scalar to the hardware reciprocal (v_rcp_f32, 1 ULP) and sqrt to v_sqrt_f32 (1 ULP);
 *   - RandomValueNormalDistribution's log to v_log_f32 x ln 2 and its cos(2 pi u) to v_cos_f32(u).
 * Unchanged: the PCG random stream, every integer decision, the traversal order, the slab test, exp in the absorption
 * term, the primary ray, the frame accumulation, and the display step of WCPT_PAYLOAD_DISPLAY_RGBA8 (the exact function
 * of the accumulated value). These always run exact, whatever the option says, and wcpt_last_arith then reports 0: the
 * wavefront kernels (also when WCPT_KERNEL_AUTO resolves to them), wcpt_render_counters (it counts the reference
 * algorithm's work), the diagnostics modes and wcpt_composite.
 * What to expect, compared with the exact mode (= the CPU oracle) on the same inputs: a fast image is deterministic -- the
 * same bits for the same frame on every tile order, stack kind, row split, frame overlap, primary-cache state and group
 * layout, fast against fast -- and per pixel either close to the exact one (every channel within 1e-5 * max(1, |exact|))
 * or diverged, where a rounding difference flipped a hit, a refraction or a take and the path went elsewhere. Stated
 * tolerance, checked by tests/test_gpu_arith.py on the Cornell box, the dielectric and the reference's scenes: at most
 * 0.5 % of a frame's pixels diverge, the median of |fast - exact| / max(1, |exact|) over all channels is <= 1e-6, and
 * finiteness matches. Measured on the MI355X: 0.06-0.26 % of the pixels diverged on those cases, 0.008 % of a 1920x1080
 * Cornell frame and 0.36 % of the reference's scene at 1920x1080; median 0 (more than half the values are bit-equal);
 * DESIGN.md section 4 has the tables. The thresholds of the exact mode (99.9 % of the
 * pixels within 1e-5, mean <= 1e-4) do not hold: a CPU oracle rebuilt with contraction allowed misses them too.
 * Any other value returns WCPT_ERROR_INVALID_ARGUMENT and leaves the option as it was. Accepting a value restarts the
 * cached frame preparation and drops the primary cache (a cached record belongs to the arithmetic that found it); an
 * application should also restart accumulation (renderedFramesCount = 0) unless it wants frames of both kinds blended.
 * In a group the option is set per rank (wcpt_group_context); all ranks must set the same value, or the presented
 * frame mixes rows of both kinds. Added under ABI 4. */
#define WCPT_OPTION_ARITH 17
#define WCPT_ARITH_EXACT 0
#define WCPT_ARITH_FAST  1

/* ---- POD types with the reference byte layouts -------------------------------------------------- */

/* SceneData — pathTracer.comp:10-22 == PathTracingRenderer.jai:38-51. 164 bytes.
 * Matrices are column-major (GLSL mat4), as the Jai host uploads them after transpose()
 * (PathTracingRenderer.jai:28,33). */
typedef struct wcpt_scene_data {
    float    inverseProjection[16]; /*   0 */
    float    inverseView[16];       /*  64 */
    float    position[3];           /* 128 */
    uint32_t maxBounceCount;        /* 140  (Jai default 3) */
    uint32_t samples;               /* 144  (Jai default 1) */
    uint32_t sphereCount;           /* 148 */
    uint32_t drawCommandCount;      /* 152 */
    uint32_t renderedFramesCount;   /* 156 */
    uint32_t boxID;                 /* 160  (unused by the kernel) */
} wcpt_scene_data;

/* Material — pathTracer.comp:35-47 == PathTracingRenderer.jai:58-70. 60 bytes. */
typedef struct wcpt_material {
    uint32_t type;                  /*  0  WCPT_MATERIAL_* (Jai default METAL) */
    float    albedo[3];             /*  4 */
    float    emission[3];           /* 16 */
    float    emissionStrength;      /* 28  (Jai default 0) */
    float    metallic;              /* 32  (unused by the kernel) */
    float    roughness;             /* 36 */
    float    absorption[3];         /* 40 */
    float    absorptionStrength;    /* 52  (Jai default 1) */
    float    ior;                   /* 56  (Jai default 1) */
} wcpt_material;

/* Sphere — pathTracer.comp:60-64 == PathTracingRenderer.jai:86-90. 20 bytes. */
typedef struct wcpt_sphere {
    float    position[3];
    float    radius;
    uint32_t material;
} wcpt_sphere;

/* Node — pathTracer.comp:66-72 == PathTracingRenderer.jai:125-134. 32 bytes.
 * triangleCount counts INDICES (3 per triangle); 0 means interior, whose children are at
 * leftNodeOrTriangleIndex and leftNodeOrTriangleIndex+1. */
typedef struct wcpt_node {
    float    min[3];
    float    max[3];
    uint32_t leftNodeOrTriangleIndex;
    uint32_t triangleCount;
} wcpt_node;

/* DrawCommand — pathTracer.comp:82-87 == PathTracingRenderer.jai:135-140. The array stride is the Jai
 * size_of = 32 bytes (28 bytes of fields + 4 bytes tail padding). The three fields are device
 * addresses from wcpt_buffer_device_address(). The reference's kernel never reads indexCount; this runtime does:
 * it derives the triangle records from index positions [0, indexCount), so indexCount must not exceed the index
 * buffer (checked for context buffers: wcpt_render returns WCPT_ERROR_INVALID_ARGUMENT), and vertex indices past a
 * context vertex buffer give a triangle that is never hit. Write draw commands through wcpt_buffer_upload, or see
 * WCPT_OPTION_TRIANGLE_CACHE.
 * Each address may lie anywhere inside a context buffer (a sub-allocation of an arena, a second mesh stored behind the
 * first), subject to its alignment: bvhBuffer a multiple of 16 bytes (the kernels load a node as two 16-byte rows),
 * vertexBuffer and indexBuffer multiples of 4 (positions and indices are read as 32-bit words, a position as three of
 * them). The bounds above then count from the address to the end of its buffer. */
typedef struct wcpt_draw_command {
    uint64_t vertexBuffer;          /* -> float[3] positions, stride 12 */
    uint64_t indexBuffer;           /* -> uint32 indices (BVH-permuted) */
    uint64_t bvhBuffer;             /* -> wcpt_node[] */
    uint32_t indexCount;
    uint32_t _pad;
} wcpt_draw_command;

/* Camera — PathTracingRenderer.jai:6-20 (the Jai Matrix4s are stored here already in the column-major
 * order the shader reads). */
typedef struct wcpt_camera {
    float position[3];
    float direction[3];
    float yaw;
    float pitch;
    float fov;                      /* vertical, degrees (Jai default 90) */
    float projection[16];
    float view[16];
    float inverseProjection[16];
    float inverseView[16];
} wcpt_camera;

/* Per-frame work counters of the reference algorithm; exact integers. */
typedef struct wcpt_counters {
    uint64_t pixels;          /* pixels rendered                                                   */
    uint64_t segments;        /* Intersect() calls = ray segments (the "rays" of Mray/s)          */
    uint64_t sphere_tests;    /* raySphereIntersect calls                                          */
    uint64_t node_pops;       /* BVH nodes popped from the stack (reference :158-159)              */
    uint64_t interior_visits; /* interior nodes whose two children were fetched (:183-184)        */
    uint64_t triangle_tests;  /* rayTriangleIntersect calls (:170)                                 */
    uint64_t hits;            /* segments that hit (material fetched, :251)                        */
    uint64_t draw_fetches;    /* DrawCommand fetches (:153)                                        */
    /* SIMD-efficiency diagnostics of this implementation (not reference work; 0 from the oracle):
     * per phase, wave-steps (a wave executed the step with >= 1 lane) and lane-steps (lanes that did).
     * lane/(64*wave) is the fraction of the 64 lanes doing useful work in that phase. */
    uint64_t wave_interior_steps, lane_interior_steps;
    uint64_t wave_triangle_steps, lane_triangle_steps;
    uint64_t wave_segment_steps, lane_segment_steps;
    /* The reference's traversal stack is `uint nodeStack[32]` (pathTracer.comp:151), pushed with the root (:155) and
     * both children of every interior node that survives its box test (:192-198). Counted exactly for the same frame
     * (ABI version 2): segments in which the reference writes nodeStack[32] or beyond -- undefined behaviour in the
     * reference, whose result for those rays has no reference meaning -- and the deepest stack the reference reaches
     * (entries after a push; UINT64_MAX if the tree was too deep to track, > 64 levels). This implementation's own
     * stack (48 entries, far children only) is unaffected by either. */
    uint64_t ref_stack_overflow_segments;
    uint64_t ref_stack_max;
} wcpt_counters;

/* Host mesh produced by the OBJ loader (ModelLoader.jai:60-141) or a scene generator. Memory is owned
 * by the library; release with wcpt_mesh_free. */
typedef struct wcpt_mesh {
    float*    positions;      /* vertex_count * 3 floats */
    uint32_t  vertex_count;
    uint32_t* indices;        /* index_count uint32 */
    uint32_t  index_count;
} wcpt_mesh;

/* Host scene (geometry + materials + spheres + camera). Owned by the library; wcpt_scene_free. */
typedef struct wcpt_scene {
    wcpt_mesh      mesh;
    wcpt_material* materials;
    uint32_t       material_count;
    wcpt_sphere*   spheres;
    uint32_t       sphere_count;
    wcpt_camera    camera;
} wcpt_scene;

typedef struct wcpt_context wcpt_context;
typedef uint64_t wcpt_buffer;      /* 0 is never a valid handle */

/* ---- library / context ---------------------------------------------------------------------------- */
int         wcpt_abi_version(void);
/* Identity of the sources and compile flags that decide this build's kernels and their launches (a short hash; the
 * multi-device group's exchange code and this header's comments are left out): measurements recorded against one
 * build (e.g. a counter profile) can tell whether they describe the kernels of the library that is loaded. */
const char* wcpt_build_id(void);
int         wcpt_device_count(int* count);
/* The PCI bus id of a device ("dddd:bb:dd.f", NUL-terminated in out[0..len)): identifies a GPU across processes that
 * see different device ordinals (e.g. a launcher that makes one device visible per process). */
int         wcpt_device_pci_bus_id(int device, char* out, int len);
int         wcpt_create(int device, wcpt_context** out_ctx);
int         wcpt_destroy(wcpt_context* ctx);                       /* Deinit, PathTracingRenderer.jai:473 */
const char* wcpt_last_error(const wcpt_context* ctx);              /* ctx may be NULL: last global error */
int         wcpt_set_stream(wcpt_context* ctx, void* hip_stream);  /* NULL: the context's own stream     */
int         wcpt_set_kernel(wcpt_context* ctx, int variant);       /* WCPT_KERNEL_*                       */
int         wcpt_last_kernel(wcpt_context* ctx, int* variant);     /* what the last render ran (AUTO resolved) */
int         wcpt_set_option(wcpt_context* ctx, int option, int value); /* WCPT_OPTION_*                   */
/* The arithmetic the last wcpt_render really ran (WCPT_ARITH_*): WCPT_ARITH_FAST only after a megakernel render with
 * WCPT_OPTION_ARITH set to it; 0 before any render. Host only. Added under ABI 4. */
int         wcpt_last_arith(wcpt_context* ctx, int* arith);

/* ---- device buffers (BufferManager.jai) ------------------------------------------------------------ */
int      wcpt_buffer_alloc(wcpt_context* ctx, uint64_t bytes, wcpt_buffer* out);
int      wcpt_buffer_upload(wcpt_context* ctx, wcpt_buffer buf, const void* src, uint64_t bytes,
                            uint64_t offset);  /* grows (reallocates) when offset+bytes > size, like :53-54 */
int      wcpt_buffer_download(wcpt_context* ctx, wcpt_buffer buf, void* dst, uint64_t bytes,
                              uint64_t offset);
int      wcpt_buffer_size(wcpt_context* ctx, wcpt_buffer buf, uint64_t* out_bytes);
uint64_t wcpt_buffer_device_address(wcpt_context* ctx, wcpt_buffer buf); /* 0 on error */
int      wcpt_buffer_free(wcpt_context* ctx, wcpt_buffer buf);

/* ---- output image (CreateScreen / Resize) --------------------------------------------------------- */
/* Frame sizes. The frame may be any width x height >= 1 of 32 bits, also one of 2^32 pixels or more: a pixel's seed is
 * pcg_hash(x + y * width + renderedFramesCount * 719393) in 32-bit arithmetic, wrapping as the reference's uint does
 * (pathTracer.comp:304), for every renderedFramesCount up to 0xFFFFFFFF (where the reference's 1 / float(count + 1) is a
 * division by zero and the accumulated RGB is NaN, here too). What is limited is what one context holds: its rows
 * (the whole frame, or the rows named by wcpt_set_row_range / wcpt_set_row_stripes) are rendered in 8x8 tiles of 64
 * lanes and may cover at most 2^32 - 64 lanes, ceil(width / 8) * ceil(rows / 8) * 64 -- an image of just under 64 GiB.
 * wcpt_render and wcpt_render_counters of more are WCPT_ERROR_INVALID_ARGUMENT, with a message, before anything is
 * launched; the context stays usable (name fewer rows). A larger frame is rendered in row blocks or stripes: rows named
 * before the first wcpt_create_screen are honoured by it, so only they are allocated.
 * The context-owned image starts as zeros (the reference's is undefined; its editor blends frame 1 with it). */
int      wcpt_create_screen(wcpt_context* ctx, uint32_t width, uint32_t height);
int      wcpt_resize(wcpt_context* ctx, uint32_t width, uint32_t height);
/* Row-block shard: this context renders and stores only rows [y0, y0+rows) of the width x height
 * frame (global pixel indices and seeds unchanged). rows == 0 resets to the full frame. */
int      wcpt_set_row_range(wcpt_context* ctx, uint32_t y0, uint32_t rows);
/* Interleaved row stripes (SURVEY.md §8(e)'s fallback when static blocks cap the scaling): this context renders
 * `rows` rows of the frame -- stripes of `stripe` rows every `period` rows, the first starting at frame row y_first,
 * the last possibly short -- and stores them back to back ([rows][width]): local row ly is frame row
 * y_first + ly + (ly / stripe) * (period - stripe). Seeds and pixel indices stay global (pathTracer.comp:304), so the
 * rows are bit-identical to a whole-frame render's. `stripe` is a power of two (1..32768), period >= stripe;
 * stripe == 0 is wcpt_set_row_range(y_first, rows). wcpt_row_stripes gives rank r of n its (y_first, rows) for
 * period = n * stripe. Added under ABI 4. */
int      wcpt_set_row_stripes(wcpt_context* ctx, uint32_t y_first, uint32_t rows, uint32_t stripe, uint32_t period);
uint64_t wcpt_image_device_ptr(wcpt_context* ctx);                 /* float4[rows][width], pitch width*16 */
/* Render into caller-owned device memory (e.g. a torch tensor handed to RCCL, or imported interop memory)
 * instead of the context's own image. `bytes` must hold width*rows*16. device_ptr == 0 reverts to the
 * context-owned image. The caller keeps ownership. device_ptr must be 16-byte aligned (the kernels store float4
 * texels); one that is not is WCPT_ERROR_INVALID_ARGUMENT and the image in use stays. */
int      wcpt_set_external_image(wcpt_context* ctx, uint64_t device_ptr, uint64_t bytes);
/* Gather payload written by the render itself: every wcpt_render also stores each pixel it
 * finishes into caller-owned device memory at `device_ptr`, row-major [rows][width], in payload format `channels`:
 *   WCPT_PAYLOAD_RGB32F (3)  float RGB, the accumulation image's values (alpha is always 1.0, pathTracer.comp:323);
 *   WCPT_PAYLOAD_RGBA32F (4) float RGBA, the accumulation image's values (16-byte aligned);
 *   WCPT_PAYLOAD_DISPLAY_RGBA8 (8) the display step of composite.comp:36-53 (gamma 1/2.2 + PBR Neutral, UNORM8 as
 *     wcpt_composite's RGBA8) of the accumulated value, 4 B/px: a presented multi-device frame at a quarter of the
 *     float payload's bytes, with no separate composite pass.
 * A multi-GPU host points it at the buffer it hands to the collective, so no copy kernel sits between the render and
 * the gather. `bytes` must hold width*rows*(bytes per pixel) at render time. device_ptr == 0 turns it off. Takes
 * effect for the next render; no synchronisation. The caller keeps ownership. */
#define WCPT_PAYLOAD_RGB32F        3
#define WCPT_PAYLOAD_RGBA32F       4
#define WCPT_PAYLOAD_DISPLAY_RGBA8 8
int      wcpt_set_gather_output(wcpt_context* ctx, uint64_t device_ptr, uint64_t bytes, uint32_t channels);
int      wcpt_readback(wcpt_context* ctx, float* dst, uint64_t bytes);
int      wcpt_image_upload(wcpt_context* ctx, const float* src, uint64_t bytes); /* seed accumulation */

/* ---- display step after the path (composite.comp:3-54) ------------------------ */
/* Gamma 1/2.2 + PBR Neutral tonemap of the accumulation image (this context's rows) into caller-owned device
 * memory at `dst` (e.g. wcpt_buffer_device_address of a buffer of width*rows*16 or *4 bytes). Asynchronous on
 * the context's stream. RGBA32F is what composite.comp stores; RGBA8 (UNORM, round to nearest) is the display
 * format (4x fewer bytes for readback or a multi-GPU gather). */
#define WCPT_COMPOSITE_RGBA32F 0
#define WCPT_COMPOSITE_RGBA8   1
int      wcpt_composite(wcpt_context* ctx, uint64_t dst, int format);

/* ---- bloom for the display step (bloom.comp, composite.comp:44-45). Added under ABI 4. ----------------- */
/* The reference's bloom.comp builds a glow around whatever exceeds `threshold` (soft knee `knee`) in a pyramid of at
 * most `levels` levels below the frame, and composite.comp adds it before gamma and the tonemap when its Bloom flag is
 * set. The reference's host dispatches neither, so the chain of the four modes is fixed here: level l of a width x
 * height frame has max(1, width >> (l + 1)) x max(1, height >> (l + 1)) texels; `levels` is clipped to
 * 1 + floor(log2(min(w_0, h_0))); prefilter the image into level 0, downsample level by level, upsample back adding
 * each level, and add the sampled level 0 to the image in the display step. The sampler (linear, clamp to edge), GLSL's
 * min / max for NaN and the order of every sum are defined in csrc/wcpt_bloom.h; DESIGN.md section 8 has the protocol.
 * Callers' defaults: threshold 1.0, knee 0.1, levels 6. */
typedef struct wcpt_bloom_params {
    float    threshold;
    float    knee;     /* finite, > 0 */
    uint32_t levels;   /* 2..12 requested; fewer are built on a small frame */
    uint32_t _pad;
} wcpt_bloom_params;
/* Host only: the clipped level count and each level's size (`w` and `h` are arrays of 16). A request outside 2..12 or
 * a frame that admits fewer than 2 levels (its half-resolution base is below 2 texels in width or height) returns
 * WCPT_ERROR_INVALID_ARGUMENT and writes nothing. */
int      wcpt_bloom_levels(uint32_t width, uint32_t height, uint32_t requested, uint32_t* levels, uint32_t* w,
                           uint32_t* h);
/* wcpt_composite with the Bloom branch taken: asynchronous on the context's stream, same `dst` and `format`. It reads
 * the accumulation image and never writes it; both pyramids are the context's (allocated by the first call, laid out
 * again when the screen size changes, freed by wcpt_destroy). Like wcpt_composite it first orders the stream after both
 * frame-overlap pipes, keeps the primary cache and the frame preparation, always runs exact and leaves wcpt_last_arith
 * alone. WCPT_ERROR_INVALID_ARGUMENT, with nothing written or launched: a null `p`, a threshold or knee that is not
 * finite, knee <= 0, levels outside 2..12, a frame that admits fewer than 2 levels, what wcpt_composite refuses about
 * `dst` and `format`, and a context that does not hold the whole frame (wcpt_set_row_range or wcpt_set_row_stripes in
 * effect): bloom reads neighbouring rows, and neither halos for row blocks nor a bloom in a group's display payload
 * (WCPT_PAYLOAD_DISPLAY_RGBA8) are provided. */
int      wcpt_composite_bloom(wcpt_context* ctx, uint64_t dst, int format, const wcpt_bloom_params* p);
/* The same result computed on the CPU by the same arithmetic (csrc/wcpt_bloom.h) from a float4 image of width x height
 * pixels: RGBA32F into `out_rgba32f` and RGBA8 into `out_rgba8`; either may be NULL. No GPU needed. Refuses as
 * wcpt_composite_bloom does (and a null image), writing nothing. */
int      wcpt_bloom_host(const float* rgba, uint32_t width, uint32_t height, const wcpt_bloom_params* p,
                         float* out_rgba32f, uint8_t* out_rgba8);

/* ---- dispatch ---------------------------------------------------------------------------------------- */
/* The push block of pathTracer.comp:90-95 minus `sdp`: SceneData travels by value. Asynchronous on the
 * context's stream; the caller owns renderedFramesCount sequencing (PathTracingRenderer.jai:423). */
int      wcpt_render(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t materials,
                     uint64_t spheres, uint64_t draw_commands);
int      wcpt_sync(wcpt_context* ctx);
/* How many renders of the context stored (*writes) and read (*reads) the primary cache (WCPT_OPTION_PRIMARY_CACHE)
 * since it was created; either pointer may be null. Host only. Added under ABI 4. */
int      wcpt_primary_cache_stats(wcpt_context* ctx, uint64_t* writes, uint64_t* reads);
/* How many renders of the context ran as two launches (WCPT_OPTION_MK_SPLIT) since it was created. Host only. Added
 * under ABI 4. */
int      wcpt_mk_split_stats(wcpt_context* ctx, uint64_t* renders);
/* How many renders of the context ran on the kernels that walk a tiny tree, with the draw's tree classified as one
 * (WCPT_OPTION_MK_TINY_TREE), since it was created: a count of renders that selected the walk, not of waves. Host only. Added under ABI 4. */
int      wcpt_mk_tiny_tree_stats(wcpt_context* ctx, uint64_t* renders);
/* What the context's last wavefront launch did (wcpt_render or wcpt_render_counters on WCPT_KERNEL_WAVEFRONT): the plan
 * of csrc/wf_plan.h as it was carried out, the inputs it was made from, and per pipeline the trace instance that was
 * really launched. Read-only and host only: it queues nothing and joins nothing, so a frame-overlap continuation goes
 * on. All zeros (launches == 0) before the first wavefront launch. Codes are csrc/wf_plan.h's wf_variant_code
 * numbering: an instance's (count, diag, geo, ldsn, persist). Added under ABI 4. */
#define WCPT_WF_MAX_PIPES 4
#define WCPT_WF_NO_VARIANT 0xFFFFFFFFu /* variant_code of a pipeline whose trace was not launched */
typedef struct wcpt_wf_pipe_info {
    uint32_t variant_code; /* of the instance handed to the dispatcher at this pipeline's (last) trace launch */
    uint32_t dispatches;   /* trace launches of this pipeline in this frame: iters per-bounce, 1 persistent */
    uint32_t tiles;        /* 8x8 tiles of the pipeline, */
    uint32_t paths;        /* its path slots */
    uint32_t iters;        /* and the plan's trace/shade iterations */
} wcpt_wf_pipe_info;
typedef struct wcpt_wf_plan_info {
    uint64_t launches;     /* wavefront launches of the context since it was created, this one included */
    int32_t  mode;         /* 0 render, 1 counting, 2 diagnostics */
    int32_t  ok;           /* 0: the frame's lanes or pixels do not fit 32 bits; nothing was launched */
    int32_t  empty;        /* 1: no pixels; nothing was launched */
    int32_t  persist;      /* 1: the pipelines ran the path-persistent trace */
    uint32_t K;            /* pipelines */
    uint32_t trace_grid;   /* waves of one pipeline's per-bounce trace */
    uint32_t shade_grid;   /* blocks of the shade kernel */
    uint32_t persist_grid; /* waves of one pipeline's persistent trace, 0 without it */
    int32_t  continued;    /* 1: under the frame overlap the pipelines continued behind the previous frame's unjoined */
    int32_t  sort;         /* 1: the ray sort ran (the option, and there are draws to sort by) */
    wcpt_wf_pipe_info pipe[WCPT_WF_MAX_PIPES]; /* [0, K) */
    /* the inputs the plan was made from */
    uint32_t base_code;    /* of the instance the launch selected, whose occupancy sizes the trace grid */
    uint32_t width, rows;  /* the context's rows of the frame */
    uint32_t samples, max_bounce;
    int32_t  wf_fetch, wf_persist, pipes; /* the options as the launch read them */
    int32_t  overlap;      /* WCPT_OPTION_FRAME_OVERLAP as the runtime allowed it for this launch */
    int32_t  cus;          /* compute units of the device */
    int32_t  trace_bpc;    /* blocks per compute unit of the base instance */
    int32_t  persist_bpc;  /* ... of the persistent instance; 0 where the launch was not eligible for it */
} wcpt_wf_plan_info;
int      wcpt_wf_last_plan(wcpt_context* ctx, wcpt_wf_plan_info* out);
/* Same frame through the instrumented kernel: counts the reference algorithm's work.
 * Does not write the image. Synchronous. */
int      wcpt_render_counters(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t materials,
                              uint64_t spheres, uint64_t draw_commands, wcpt_counters* out);

/* ---- what a pixel shows: the primary-hit buffer and the pick. Added under ABI 4. ------------------------ */
/* One record per pixel: what the reference's Intersect (pathTracer.comp:135-211) leaves in its record for the pixel's
 * primary ray, in exact arithmetic, with the identity of the primitive. The spheres are tested in index order, then the
 * draw commands in order, each by the reference's traversal; a closer hit replaces the record only on strict `<`, so
 * on equal t the earlier primitive in that order stays. p is not stored: it is origin + t * direction on these bits. Of
 * `scene` only inverseProjection, inverseView, position, sphereCount and drawCommandCount are read, and no material
 * buffer is needed. Both calls always run exact, whatever WCPT_OPTION_ARITH says. An editor selects the object under a
 * click with the pick; the buffer (depth, normal, identity per pixel) is the guide image of an outline or of the
 * denoiser below (wcpt_composite_denoise). */
#define WCPT_HIT_MISS     0u
#define WCPT_HIT_SPHERE   1u
#define WCPT_HIT_TRIANGLE 2u
#define WCPT_HIT_KIND_MASK 3u
#define WCPT_HIT_FRONT    0x80000000u
typedef struct wcpt_primary_hit {
    float    direction[3];  /*  0  the pixel's primary ray direction (pathTracer.comp:290-302)                       */
    float    t;             /* 12  hit distance; the kernels' kInfinity (bits 0x7F7FFFFF) on a miss                  */
    float    normal[3];     /* 16  as Intersect returns it: flipped towards the ray; zeros on a miss                 */
    uint32_t kind;          /* 28  WCPT_HIT_* in bits 0-1, bit 31 (WCPT_HIT_FRONT) = front: dot(direction, normal)
                                   was < 0 before the flip                                                           */
    uint32_t material;      /* 32  the sphere's material; 0 for a triangle (:175) and for a miss                     */
    uint32_t index;         /* 36  sphere index, or the triangle's number in its draw's permuted index buffer (index
                                   position / 3); 0 on a miss                                                        */
    uint32_t draw;          /* 40  draw command of a triangle hit; 0 otherwise                                       */
    uint32_t _pad;          /* 44  written as 0                                                                      */
} wcpt_primary_hit;
/* The context's rows back to back, [rows][width] records, into caller-owned device memory `dst` (16-byte aligned,
 * `bytes` >= width * rows * 48); a row range and row stripes are honoured with the row map a render uses. Asynchronous
 * on the context's stream; like wcpt_composite it first orders the stream behind both frame-overlap pipes. A refused
 * far-child push (a tree deeper than the traversal stack) sets WCPT_ERROR_STACK_OVERFLOW for the next wcpt_sync, as a
 * render does.
 * wcpt_pick is the same kernel on a one-pixel window: (x, y) is any pixel of the frame, whether or not the context holds
 * its row. Synchronous; fills *out on the host and returns a stack overflow itself.
 * Neither call touches the accumulation image, the gather output, wcpt_last_kernel, wcpt_last_arith, the primary cache or
 * its statistics, or the split and tiny-tree counters. Both share a render's frame preparation: a prepared scene is not
 * prepared again, and the next render's preparation still hits.
 * WCPT_ERROR_INVALID_ARGUMENT (WCPT_ERROR_NO_SCREEN without a screen), with nothing launched or written: a null scene, a
 * frame that is not renderable ("Frame sizes"), sphereCount > 0 with null spheres, drawCommandCount > 0 with null draw
 * commands, a draw command a render refuses, a null, misaligned or too small `dst`, a null `out`, x >= width or
 * y >= height. */
int      wcpt_trace_primary(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t spheres,
                            uint64_t draw_commands, uint64_t dst, uint64_t bytes);
int      wcpt_pick(wcpt_context* ctx, const wcpt_scene_data* scene, uint64_t spheres, uint64_t draw_commands,
                   uint32_t x, uint32_t y, wcpt_primary_hit* out);

/* ---- guided denoise for the display step. Added under ABI 4. -------------------------------------------------- */
/* An interactive session is mostly one-sample frames (the reference's editor restarts the accumulation on every camera
 * move and gizmo drag). wcpt_composite_denoise is wcpt_composite with an edge-avoiding a-trous wavelet filter (Dammertz
 * et al. 2010) between the accumulation image and the display step, guided by the primary-hit records: `iterations`
 * passes of a 5x5 B3-spline kernel whose taps lie 1, 2, 4, ... pixels apart; a tap counts only when it shows the same
 * surface as the pixel -- the same sphere, the same draw command, or the sky -- and is weighted down by its colour
 * difference (sigma_color), its normal difference (sigma_normal) and its distance from the pixel's tangent plane relative
 * to the pixel's hit distance (sigma_depth). The reference has no textures, so a surface's albedo is constant and the
 * identity test does what albedo demodulation does elsewhere. The reference has no denoiser: csrc/wcpt_denoise.h fixes the
 * rule and the order of every operation; DESIGN.md section 8 has what it is worth. Callers' defaults: 5, 4.0, 0.5, 0.05. */
typedef struct wcpt_denoise_params {
    uint32_t iterations;   /* 1..6 */
    float    sigma_color;  /* > 0, not NaN; +inf turns the colour term off */
    float    sigma_normal; /* finite, > 0 */
    float    sigma_depth;  /* finite, > 0: relative to the pixel's hit distance */
} wcpt_denoise_params;
/* `guide` is caller-owned device memory (16-byte aligned, `guide_bytes` >= width * height * 48) holding the
 * [height][width] records wcpt_trace_primary wrote for the camera and scene of the accumulated frames; the call traces
 * nothing and needs no scene. Asynchronous on the context's stream, same `dst` and `format` as wcpt_composite. Like
 * wcpt_composite it first orders the stream behind both frame-overlap pipes; it reads the accumulation image and never
 * writes it, leaves the primary cache, the frame preparation, wcpt_last_kernel, wcpt_last_arith and every counter alone,
 * and always runs exact. Its scratch (64 bytes per pixel) is the context's: allocated by the first call, grown on a
 * larger screen, freed by wcpt_destroy. A guide that does not belong to the image gives a wrong picture but never an
 * access outside the two buffers: guide contents are only compared and multiplied, never used as an index.
 * WCPT_ERROR_NO_SCREEN without a screen. WCPT_ERROR_INVALID_ARGUMENT, with nothing launched or written: a null `p`,
 * iterations outside 1..6, a sigma that is NaN, <= 0 or (except sigma_color) infinite, a null guide, one that is not
 * 16-byte aligned, guide_bytes below width * height * 48, a guide inside a context buffer too small for that, what
 * wcpt_composite refuses about `dst` and `format`, and a context that does not hold the whole frame (wcpt_set_row_range
 * or wcpt_set_row_stripes in effect): the filter reads neighbouring rows, as bloom does. Not provided: denoise and bloom
 * in one call, halos for row blocks, a denoised group payload (WCPT_PAYLOAD_DISPLAY_RGBA8). */
int      wcpt_composite_denoise(wcpt_context* ctx, uint64_t guide, uint64_t guide_bytes, uint64_t dst, int format,
                                const wcpt_denoise_params* p);
/* The same result computed on the CPU by the same arithmetic (csrc/wcpt_denoise.h) from a float4 image and the records
 * of width x height pixels: RGBA32F into `out_rgba32f` and RGBA8 into `out_rgba8`; either may be NULL. No GPU needed.
 * Refuses as wcpt_composite_denoise does about `p` (and a null image, a null guide, a frame without pixels), writing
 * nothing. */
int      wcpt_denoise_host(const float* rgba, const wcpt_primary_hit* guide, uint32_t width, uint32_t height,
                           const wcpt_denoise_params* p, float* out_rgba32f, uint8_t* out_rgba8);

/* ---- temporal reprojection for the display step. Added under ABI 4. ---------------------------------------------- */
/* While anything moves, every displayed frame is a fresh one-sample image and every earlier frame is thrown away, although
 * the surfaces on screen are mostly those of a frame ago. wcpt_composite_temporal is wcpt_composite (or, with `d`,
 * wcpt_composite_denoise) of a blend of the accumulation image with the previous result, looked up where each pixel's
 * surface point was a frame ago: the temporal half of an SVGF-style pipeline. A sequence is the calls between two restarts
 * of the accumulation. A restart call reprojects each pixel's hit point (the sky: its direction) into the previous
 * sequence's frame, gathers the four surrounding texels of the previous output that show the same surface (the same
 * identity, a normal within normal_min, a distance from the pixel's tangent plane within depth_tol of its hit distance),
 * and keeps their weighted mean as the sequence's `base` with the samples it counts, at most max_history. Every call blends
 * base with the accumulation image by the two sample counts, so a still camera converges as it does without this stage.
 * csrc/wcpt_temporal.h fixes the rule and the order of every operation; DESIGN.md section 8 has what it is worth and the
 * limit the reference's seed sets. Callers' defaults: 32, 0.9, 0.05. */
typedef struct wcpt_temporal_params {
    uint32_t max_history;  /* 1..65536: the samples a history may count */
    float    normal_min;   /* finite, in [-1, 1]: the least dot product of the two normals */
    float    depth_tol;    /* finite, > 0: relative to the pixel's hit distance */
    uint32_t _pad;         /* ignored */
} wcpt_temporal_params;
/* `scene` is the scene data of the accumulated frames (of it inverseProjection, inverseView and position are read, the
 * fields wcpt_trace_primary reads: the reprojection inverts what the rays did, whatever matrix convention the host has),
 * `frames` the number of samples in the accumulation image (the last render's renderedFramesCount + 1), `guide` and
 * `guide_bytes` the records of wcpt_trace_primary for that camera as for wcpt_composite_denoise. restart != 0 says that the
 * accumulation restarted since the previous call and `guide` is the new sequence's guide; with restart == 0, `guide` must be
 * the sequence's guide again and only the denoise reads it. The first call, and the first after wcpt_temporal_reset,
 * wcpt_create_screen, wcpt_resize or a change of the context's rows, is a restart without history whatever `restart` says.
 * `d` NULL: the blend goes through the display step as wcpt_composite does it; otherwise through wcpt_composite_denoise's
 * filter first. Asynchronous on the context's stream, same `dst` and `format` as wcpt_composite; like wcpt_composite it first
 * orders the stream behind both frame-overlap pipes. It reads the accumulation image and never writes it, leaves the primary
 * cache, the frame preparation, wcpt_last_kernel, wcpt_last_arith and every counter alone, and always runs exact. Its
 * scratch (120 bytes per pixel: the previous output with its lengths and packed guide twice, and base; with `d` also
 * wcpt_composite_denoise's 64) is the context's: allocated by the first call, laid out again on a new screen size, freed by
 * wcpt_destroy. A guide or a camera that does not belong to the image gives a wrong picture but never an access outside the
 * buffers: guide words are only compared and multiplied, and a tap's position comes from a range-checked coordinate.
 * WCPT_ERROR_NO_SCREEN without a screen. WCPT_ERROR_INVALID_ARGUMENT, with nothing launched and no state changed: a null
 * `scene` or `t`, max_history outside 1..65536, a normal_min that is NaN or outside [-1, 1], a depth_tol that is NaN, <= 0 or
 * infinite, frames == 0, a camera whose inverseProjection or the upper-left 3x3 of whose inverseView is singular or whose
 * corner pixels do not come back to their centres within 1e-3 pixel (a projection that is not a plain perspective), what
 * wcpt_composite_denoise refuses about `guide`, `dst`, `format` and `d`, and a context that does not hold the whole frame.
 * Not provided: halos for row blocks, a temporal group payload, bloom in the same call. */
int      wcpt_composite_temporal(wcpt_context* ctx, const wcpt_scene_data* scene, uint32_t frames, int restart,
                                 uint64_t guide, uint64_t guide_bytes, uint64_t dst, int format,
                                 const wcpt_temporal_params* t, const wcpt_denoise_params* d);
/* Drops the history: the next wcpt_composite_temporal is a restart without history. For what the records cannot see: a
 * material, light or mesh change. Host only. */
int      wcpt_temporal_reset(wcpt_context* ctx);
/* One call of wcpt_composite_temporal's state sequence on the CPU by the same arithmetic (csrc/wcpt_temporal.h), stateless:
 * the caller carries the state. `rgba` is the accumulation image (float4), `guide` and `scene` its records and scene data.
 * restart != 0: `base` (3 floats per pixel) and `n_b` (1 float per pixel) are written, from the history -- the previous
 * call's out_rgba and out_length with the records and scene data of the sequence they belong to; a NULL hist_rgba means no
 * history and the other three are then not read -- and then blended. restart == 0: base and n_b are read (the sequence's)
 * and left as they are, and the history arguments are not read. Either way out_rgba (float4) and out_length (1 float per
 * pixel) receive the new output and its lengths; they must not alias the history. Display and denoise of out_rgba go through
 * wcpt_denoise_host or the composite of the oracle. Refuses as wcpt_composite_temporal does about `scene`, `hist_scene`,
 * `frames` and `t` (and a null image, guide or output, a history without all four parts, a frame without pixels), writing
 * nothing. No GPU needed. */
int      wcpt_temporal_host(const float* rgba, uint32_t frames, int restart, const wcpt_primary_hit* guide,
                            const wcpt_scene_data* scene, uint32_t width, uint32_t height, const wcpt_temporal_params* t,
                            const float* hist_rgba, const float* hist_length, const wcpt_primary_hit* hist_guide,
                            const wcpt_scene_data* hist_scene, float* base, float* n_b, float* out_rgba,
                            float* out_length);

/* Wavefront trace-loop phase timers of the last wcpt_render_counters call with WCPT_OPTION_DIAGNOSTICS set
 * (s_memtime cycles summed over waves): {fetch, leaf, interior, pop, epilogue, waves, iterations, -}. */
int      wcpt_read_diagnostics(wcpt_context* ctx, uint64_t* out, uint32_t n);

/* ---- one frame on several devices ------------------------------------------------------- */
/* The reference host is one process and one thread (main.jai:185-194) driving Render (PathTracingRenderer.jai:399).
 * A group keeps that shape for N devices: one context per device, rank r rendering rows [r*H/N, (r+1)*H/N) of the
 * frame with unchanged global pixel indices and seeds (so the frame equals a one-device render bit for bit), and one
 * exchange per presented frame: the row blocks go to the root device over xGMI (blocks may differ by a row).
 *   wcpt_group_create      one process, one thread, devices[0..n) distinct device ordinals, RCCL transport
 *                          (ncclCommInitAll, rccl.h:236; grouped ncclSend/ncclRecv, rccl.h:700,722). `root` is the
 *                          rank that receives the frame.
 *   wcpt_group_create_ex   the same with a transport: WCPT_GROUP_TRANSPORT_RCCL, WCPT_GROUP_TRANSPORT_COPY
 *                          (hipMemcpyPeerAsync of each block into the root's frame, on the sending device's copy
 *                          path; a device may then be listed more than once, so an N-rank group can be rehearsed on
 *                          fewer devices: every rank still has its own context, streams and payloads), or
 *                          WCPT_GROUP_TRANSPORT_DIRECT (each render writes its block into the root's frame itself).
 *                          Status: RCCL between n > 1 distinct GPUs over xGMI is UNVERIFIED on hardware here (the
 *                          development boxes have one GPU). The one-process-per-device form (below) has run with 2,
 *                          4 and 8 ranks on one GPU over RCCL's socket transport (bench.py --rccl-rehearsal, frame verified
 *                          bit-exact); the COPY and DIRECT transports run the same bookkeeping and are tested with 2-8
 *                          ranks on one GPU.
 *   wcpt_group_unique_id / wcpt_group_create_rank   one process per device (e.g. one process per GPU under
 *                          torchrun): the root's process makes the id (ncclGetUniqueId), the host hands its 128 bytes
 *                          to every process, and each process creates its rank (ncclCommInitRank). RCCL only. All
 *                          processes then make the same wcpt_group_* calls in the same order (collective).
 *   wcpt_group_context     rank r's context (NULL for a rank of another process): upload that device's copy of the
 *                          scene with wcpt_buffer_* and set kernels/options on it, as for a single context. Owned by
 *                          the group.
 *   wcpt_group_create_screen  CreateScreen/Resize for the whole frame (each rank allocates only its row block).
 *   wcpt_group_set_output  where the presented frame goes: device memory on the root device (e.g.
 *                          wcpt_buffer_device_address of a root-context buffer) of `bytes` >= width*height*(payload
 *                          bytes per pixel), row-major, in WCPT_PAYLOAD_* format; format 0 turns presenting off (the
 *                          ranks keep accumulating their blocks), and so does dst == 0 in a one-process group. Every
 *                          process passes the same `format` and `bytes` (a process that does not hold the root ignores
 *                          `dst`), so each makes the same decision on them and on later resizes. The root renders its
 *                          own block straight into the output; the other ranks' renders write their blocks into
 *                          group-owned payload buffers (no copy pass).
 *   wcpt_group_render      Render on every rank of this process (scene by value; materials/spheres/draw_commands are
 *                          arrays of one device address per local rank, in rank order), then, with an output set,
 *                          the gather of this frame. Asynchronous, like wcpt_render. Every rank's arguments are
 *                          checked before any rank renders, so an argument error leaves every rank's accumulation as
 *                          it was. With WCPT_GROUP_OPTION_OVERLAP (default 1) each rank's transfer runs on a
 *                          communication stream of its own, ordered after that rank's render by an event, while the
 *                          next frame renders into a second payload buffer; a render waits (on the device, not the
 *                          host) only for the transfer that last read the payload it rewrites. 0: transfers run on
 *                          the render streams, in line with the renders.
 *   wcpt_group_sync        waits for every local rank's renders and transfers (and reports a traversal-stack
 *                          overflow on any of them). The presented frame is complete after it. The wait is bounded
 *                          (WCPT_GROUP_OPTION_TIMEOUT_MS): a frame whose exchange cannot complete (a peer failed or
 *                          skipped it) ends in WCPT_ERROR_DEVICE_LOST, not in a hang.
 * Errors leave the group usable, except (a) any failure once a frame's device work has started to be issued (a render
 * launch, an event, a transfer: the ranks are then out of step), and (b), in a group created with
 * wcpt_group_create_rank, an error that the other processes cannot have seen -- any wcpt_group_render error while
 * presenting, a check of the root's own `dst` (alignment, a null dst with a nonzero format), a device failure in
 * wcpt_group_create_screen / wcpt_group_set_output -- since the other processes still post their part of the next
 * exchange. The group then aborts its communicators and every later call but wcpt_group_destroy returns
 * WCPT_ERROR_DEVICE_LOST; the other processes' exchange does not complete, and their wcpt_group_sync returns
 * WCPT_ERROR_DEVICE_LOST at its timeout (or earlier, on the transport's asynchronous error). Refusals made
 * alike in every process (frame size, format, `bytes`) leave the group usable.
 * wcpt_last_error(wcpt_group_context(g, r)) or wcpt_last_error(NULL) explains an error. */
/* The row-block split itself, for a host that runs one process per device (then wcpt_set_row_range with the
 * result): rank r of n renders rows [r*height/n, (r+1)*height/n). Host-only, no device needed. */
int           wcpt_row_block(uint32_t height, uint32_t n, uint32_t rank, uint32_t* y0, uint32_t* rows);
/* The interleaved split (wcpt_set_row_stripes with period = n * stripe): rank r of n takes the stripes r, r + n,
 * r + 2n, ... of `stripe` rows; *y_first = r * stripe, *rows = the rows it holds (0 when the frame has fewer than r + 1
 * stripes). stripe == 0 is wcpt_row_block. Host-only. Added under ABI 4. */
int           wcpt_row_stripes(uint32_t height, uint32_t n, uint32_t rank, uint32_t stripe, uint32_t* y_first,
                               uint32_t* rows);
typedef struct wcpt_group wcpt_group;
#define WCPT_GROUP_TRANSPORT_RCCL 0
#define WCPT_GROUP_TRANSPORT_COPY 1
/* One process (wcpt_group_create_ex): every sender's render writes its row block straight into the root's frame over
 * xGMI (peer access, enabled at creation; refused when a sender's device cannot access the root's), so presenting a
 * frame costs no transfer, event or copy: the host issues one launch per rank. A device may be listed more than once. */
#define WCPT_GROUP_TRANSPORT_DIRECT 2
#define WCPT_GROUP_UNIQUE_ID_BYTES 128   /* == sizeof(ncclUniqueId) (rccl.h NCCL_UNIQUE_ID_BYTES) */
#define WCPT_GROUP_OPTION_OVERLAP 1
/* How a one-process group issues a frame to its devices. 1: the caller's thread issues the first local rank's share
 * (validation, render launch, events, transfer) while a host thread per other local rank issues that rank's share at the
 * same time, and wcpt_group_render returns once every share is enqueued (the API stays single-threaded for the caller;
 * threads spin ~0.2 ms between frames, then sleep). 0 (default): the caller's thread issues every rank's share in turn.
 * -1: 1 when the group's ranks span more than one device and the transport is COPY or DIRECT, else 0 (an RCCL group
 * issues all its sends and receives inside one ncclGroupStart/End from one thread unless 1 is set). Same device work
 * either way. Off by default because the threaded issue has only run with every rank on one device. Host issue per
 * frame at 8 ranks (measured on one device): COPY 95-137 us in one thread, 28-40 us with threads; DIRECT
 * 27.5 us in one thread, 13.5 us with threads. */
#define WCPT_GROUP_OPTION_THREADS 2
/* Bound on one wcpt_group_sync (and on the drain in wcpt_group_destroy), in milliseconds; 0 = wait forever; default
 * 60000 in a group of several ranks (none in a group of one). The sync polls each local rank's render and
 * communication streams (hipStreamQuery) and the communicator's asynchronous error (ncclCommGetAsyncError) instead of
 * blocking: when a peer has failed or did not post its part of a frame's exchange, the transfers never complete, so on
 * an asynchronous error or at the deadline the group aborts its communicators (ncclCommAbort), lets the aborted work
 * drain, and returns WCPT_ERROR_DEVICE_LOST (the group is then broken: every later call but wcpt_group_destroy returns
 * WCPT_ERROR_DEVICE_LOST). Pick it above the longest run of frames the host queues between two syncs. Option 3 was
 * added under ABI 4. */
#define WCPT_GROUP_OPTION_TIMEOUT_MS 3
/* Rows per interleaved stripe of the group's split: 0 (default) = contiguous row blocks (wcpt_row_block); a power of
 * two = rank r renders the stripes r, r + n, r + 2n, ... of that many rows (wcpt_row_stripes), so every rank gets rows
 * from the whole frame and a scene whose cost sits in one region no longer loads one rank. Multiples of 8 keep the
 * kernels' 8x8 tiles inside a stripe. The presented frame is the same bits either way: the root renders its stripes
 * straight into their rows of the output, RCCL blocks arrive in a root-side staging buffer and are copied to their rows
 * on the root's communication stream (hipMemcpy2DAsync), COPY senders copy their stripes to their rows, and DIRECT
 * senders write their rows themselves. Every process sets the same value; takes effect at once (the screen is laid
 * out again and accumulation restarts). Added under ABI 4. */
#define WCPT_GROUP_OPTION_ROW_STRIPE 4
typedef struct wcpt_group_info {
    int32_t nranks;            /* ranks of the group; RCCL: ncclCommCount of this process's first communicator */
    int32_t local_ranks;       /* ranks driven by this process */
    int32_t first_local_rank;
    int32_t root;
    int32_t transport;         /* WCPT_GROUP_TRANSPORT_* */
    int32_t overlap;           /* WCPT_GROUP_OPTION_OVERLAP */
    int32_t distinct_devices;  /* distinct devices among this process's ranks */
    int32_t broken;            /* 1 after a transport failure aborted the communicators */
    uint64_t frames;           /* frames rendered (and, with an output set, gathered) */
    int32_t issue_threads;     /* host threads issuing frames beside the caller's (WCPT_GROUP_OPTION_THREADS) */
    int32_t _pad;
} wcpt_group_info;
int           wcpt_group_create(const int* devices, int n, int root, wcpt_group** out);
int           wcpt_group_create_ex(const int* devices, int n, int root, int transport, wcpt_group** out);
int           wcpt_group_unique_id(uint8_t* id /* WCPT_GROUP_UNIQUE_ID_BYTES */);
int           wcpt_group_create_rank(int device, int nranks, int rank, int root, const uint8_t* id, wcpt_group** out);
int           wcpt_group_destroy(wcpt_group* g);
wcpt_context* wcpt_group_context(wcpt_group* g, int rank);
int           wcpt_group_set_option(wcpt_group* g, int option, int value);
int           wcpt_group_info_get(wcpt_group* g, wcpt_group_info* out);
int           wcpt_group_create_screen(wcpt_group* g, uint32_t width, uint32_t height);
int           wcpt_group_set_output(wcpt_group* g, int format, uint64_t dst, uint64_t bytes);
int           wcpt_group_render(wcpt_group* g, const wcpt_scene_data* scene, const uint64_t* materials,
                                const uint64_t* spheres, const uint64_t* draw_commands);
int           wcpt_group_sync(wcpt_group* g);

/* HIP runtime version the library runs on (hipRuntimeGetVersion), e.g. 70226090 for ROCm 7.2. */
int      wcpt_runtime_version(int* version);

/* ---- kernel timing (HIP events on the context's stream) -------------------------------------------- */
int      wcpt_profile_begin(wcpt_context* ctx);
int      wcpt_profile_end(wcpt_context* ctx, double* kernel_ms_total, uint32_t* launches);

/* ---- BVH build on the device ------------------------------------------------------------------------ */
/* The midpoint BVH of the triangles indices[0 .. index_count) over `vertices` (float[3] at stride 12), built on the
 * context's device from three context buffers; nothing leaves the device. Permutes `indices` in place and writes
 * nodes[0 .. *nodes_used): afterwards both hold exactly the bytes wcpt_bvh_build (below) produces from the same positions
 * and the same starting index order -- bounds, counts, leftNodeOrTriangleIndex, node numbering, permutation. The contents
 * of `nodes` past *nodes_used are unspecified. Synchronous: runs on the context's stream, behind the frame-overlap
 * pipes, and returns when its work has finished.
 * WCPT_ERROR_INVALID_ARGUMENT, with neither buffer written: an unknown handle (or one buffer passed twice);
 * index_count zero or no multiple of 3; vertex_count * 12 or index_count * 4 beyond its buffer; `nodes` smaller than
 * 2 * index_count / 3 nodes; an index >= vertex_count (found on the device by a pass that reads only the indices, before
 * any vertex is read); a referenced coordinate that is not finite -- a difference from wcpt_bvh_build, which folds NaNs
 * in index order: min as a < b ? a : b is not associative once a NaN is present, so no parallel reduction has its bits.
 * For the runtime's caches the call is a write of `indices` and `nodes`, exactly as wcpt_buffer_upload of both: a render
 * that follows needs no option change. Scratch memory (about 300 bytes per triangle) belongs to the context: allocated
 * by the first call, grown on demand, freed by wcpt_destroy. */
int      wcpt_bvh_build_device(wcpt_context* ctx, wcpt_buffer vertices, uint32_t vertex_count, wcpt_buffer indices,
                               uint32_t index_count, wcpt_buffer nodes, uint32_t* nodes_used);
/* The binned-SAH BVH, built the same way: the arguments, the synchronous contract, the scratch ownership and the meaning
 * for the runtime's caches are those of wcpt_bvh_build_device, and afterwards `indices` and nodes[0 .. *nodes_used) hold
 * exactly the bytes wcpt_bvh_build_sah (below) produces from the same positions and the same starting index order.
 * WCPT_ERROR_INVALID_ARGUMENT, with neither buffer written: everything wcpt_bvh_build_device refuses, and the inputs on
 * which wcpt_bvh_build_sah's float-to-int conversion of a bin would be undefined or which it would sort -- differences
 * from wcpt_bvh_build_sah, which accepts them:
 *   - a triangle whose centroid 0.5f * (min + max) is not finite on some axis (|min + max| overflows binary32);
 *   - a node of two or more triangles whose centroid extent on some axis is positive and not finite, or so small
 *     (below about 4.7e-38) that 16.f / extent is not finite;
 *   - a node of more than 8 triangles with a positive centroid extent in which no split has a finite cost (its box's
 *     extent overflows binary32, so every area is inf or NaN): the host builder falls back to a sort by centroid there.
 * Scratch: about 350 bytes per triangle, shared with wcpt_bvh_build_device, plus 1536 bytes per node of two or more
 * triangles on the level that has most of them (at most index_count / 6 nodes). */
int      wcpt_bvh_build_sah_device(wcpt_context* ctx, wcpt_buffer vertices, uint32_t vertex_count, wcpt_buffer indices,
                                   uint32_t index_count, wcpt_buffer nodes, uint32_t* nodes_used);
/* Refit: the vertices moved, the triangles did not. The boxes of nodes[0 .. nodes_used) are recomputed on the device from
 * the vertex buffer's current contents, bottom-up; the tree's shape -- leftNodeOrTriangleIndex, triangleCount, the index
 * order, the node numbering -- is never written. A leaf's box is the fold of a < b ? a : b / a > b ? a : b over the
 * vertices of its index range in index order from +-FLOAT32_MAX (the reference's UpdateNodeBounds), an interior node's
 * the union of its children's with the left child as the first operand. Afterwards nodes[0 .. nodes_used) holds exactly
 * the bytes wcpt_bvh_refit (below) produces; `nodes` past nodes_used, `indices` and `vertices` are untouched. Three
 * distinct context buffers; synchronous on the context's stream, behind the frame-overlap pipes, like the builds. The
 * tree may be either builder's or hand-made. Over unchanged positions a refit reproduces the builder's boxes in value,
 * and in bits except that a bound that is a zero may change its sign (the builders resolve a +0 / -0 tie by an order of
 * the triangles that the finished tree no longer holds).
 * WCPT_ERROR_INVALID_ARGUMENT, with no byte of `nodes` changed and a message that names the reason: an unknown handle
 * (or one buffer passed twice); vertex_count * 12, index_count * 4 or nodes_used * 32 beyond its buffer; nodes_used zero;
 * and whatever is not a tree over these indices, found on the device by read-only passes --
 *   - an interior node i (triangleCount 0) whose left child is not > i or whose right child left + 1 is not < nodes_used
 *     (both builders number children after their parents);
 *   - a node other than 0 that is not the child of exactly one interior node;
 *   - a leaf whose triangleCount is no multiple of 3 or whose range left + triangleCount exceeds index_count;
 *   - an index >= vertex_count anywhere in indices[0 .. index_count) (a pass that reads only the indices; no vertex is
 *     read once it has found one);
 *   - a coordinate a leaf references that is not finite.
 * A refit never improves a tree. It keeps the partition the builder chose for the old positions: after a large
 * deformation the boxes of siblings overlap and rays visit more nodes, with the same image. When to build anew
 * (wcpt_bvh_build_device, wcpt_bvh_build_sah_device) is the application's decision.
 * For the runtime's caches the call is a write of `nodes` AND of `vertices`, exactly as wcpt_buffer_upload of both. So an
 * application may deform the vertices with a kernel of its own (or a hipMemcpy) at wcpt_buffer_device_address, call the
 * refit and render with WCPT_OPTION_TRIANGLE_CACHE left at 1: the triangle records, the leaf scan, the tiny-tree flag,
 * the frame preparation and the primary cache are all re-learned. Scratch: about 40 bytes per node, shared with the
 * builds. */
int      wcpt_bvh_refit_device(wcpt_context* ctx, wcpt_buffer vertices, uint32_t vertex_count, wcpt_buffer indices,
                               uint32_t index_count, wcpt_buffer nodes, uint32_t nodes_used);

/* ---- host utilities (no GPU needed) ----------------------------------------------------------------- */
/* OBJ text -> unique (v,vt,vn) vertices + fan-triangulated indices (ModelLoader.jai:60-141). */
int      wcpt_obj_parse(const char* text, uint64_t length, wcpt_mesh* out);
int      wcpt_obj_load(const char* path, wcpt_mesh* out);
void     wcpt_mesh_free(wcpt_mesh* mesh);
/* Midpoint BVH (PathTracingRenderer.jai:147-217). Permutes `indices` in place. `nodes` must hold
 * max_nodes entries; 2*index_count/3 is always enough. */
int      wcpt_bvh_build(const float* positions, uint32_t vertex_count, uint32_t* indices,
                        uint32_t index_count, wcpt_node* nodes, uint32_t max_nodes, uint32_t* nodes_used);
/* Optional binned-SAH builder: same node format and conventions, a different tree (far
 * fewer nodes visited on large meshes). Images equal the midpoint tree's except where two triangles hit at exactly
 * the same t. Permutes `indices` into leaf order; 2*index_count/3 nodes always suffice. */
int      wcpt_bvh_build_sah(const float* positions, uint32_t vertex_count, uint32_t* indices,
                            uint32_t index_count, wcpt_node* nodes, uint32_t max_nodes, uint32_t* nodes_used);
/* The refit of wcpt_bvh_refit_device (above) on the host: the same rule, the same refusals (WCPT_ERROR_INVALID_ARGUMENT,
 * no byte of `nodes` changed, the reason in wcpt_last_error(NULL)), the same bytes. It is the byte reference of the
 * device path and the sensible choice for small meshes, where the device refit is bound by its launches. */
int      wcpt_bvh_refit(const float* positions, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                        wcpt_node* nodes, uint32_t nodes_used);
/* Camera Update (PathTracingRenderer.jai:22-36): yaw/pitch/fov/position -> matrices. */
int      wcpt_camera_update(wcpt_camera* cam, float aspect_ratio);
/* Scene generators: "default" (reference Init scene, PathTracingRenderer.jai:322-339, without a mesh),
 * "cornell" (Cornell-class box), "atrium" (deterministic Sponza-scale procedural OBJ, ~260k tris). */
int      wcpt_scene_generate(const char* name, uint32_t seed, wcpt_scene* out);
void     wcpt_scene_free(wcpt_scene* scene);
/* Scene as OBJ text (so the atrium goes through the same loader path as ModelLoader.jai). The returned
 * string is owned by the library: release with wcpt_string_free. */
int      wcpt_mesh_to_obj(const wcpt_mesh* mesh, char** out_text, uint64_t* out_length);
void     wcpt_string_free(char* text);

/* ---- self-test entry points (used by the parity tests; GPU) ---------------------------------------- */
/* Evaluates device functions on n inputs: fn 0 = pcg_hash, 1 = rand stream (4 per input),
 * 2 = log, 3 = cos, 4 = exp, 5 = sqrt (the kernels' sqrt_exact), 6 = divide(in, in2), 7 = RandomDirection (3 per input),
 * 8 = exhaustive check of the fast reciprocal (out[i] = mismatches vs IEEE 1/x over the bit patterns
 * (in[i] << 16) | k, k < 2^16), 9 = the reciprocal used by the kernels, 10/11 = as 8 over every normal /
 * every input, 12 = as 8 for the kernels' reciprocals (rcp_exact, and its packed pair form on (x, ~x)),
 * 13 = how many inputs of the block fail the fast result's class check (take the general division),
 * 14 = the two triangle acceptance forms on (u, v) = (in, in2) with t = 1 (bit 0 compares, bit 1 minimum3),
 * 15 = as 8 for the kernels' square root (sqrt_exact) against the correctly rounded sqrtf,
 * 16 = the kernels' GLSL vector / scalar on one component: in * RN(1 / in2), 17 = as 8 for the integer form of the
 * triangle take (0 < t < rec.t as bits(t) - 1 < bits(rec.t) - 1) with rec.t = in2[i].
 * The fast arithmetic mode's functions (WCPT_OPTION_ARITH), to be compared with fn 2, 3, 5, 9 and 7: 18 = log
 * (v_log_f32 x ln 2), 19 = cos(2 pi u) given u (v_cos_f32), 20 = sqrt (v_sqrt_f32), 21 = the reciprocal (v_rcp_f32),
 * 22 = RandomDirection (3 per input). Host arrays of 32-bit words. */
int      wcpt_selftest_device(wcpt_context* ctx, int fn, const uint32_t* in, const uint32_t* in2,
                              uint32_t* out, uint32_t n);
/* Evaluates the composite device functions of the render kernels, called as those kernels call them, on n items in the
 * arithmetic mode `arith` (WCPT_ARITH_EXACT or WCPT_ARITH_FAST; anything else: WCPT_ERROR_INVALID_ARGUMENT). Item i
 * reads in[i * in_words ..) and writes out[i * out_words ..); both counts must be the function's (below). Floats are
 * passed as their bit patterns; vectors as x, y, z.
 *   fn 0  rayTriangleE         in 15: origin, direction, a, b, c (edges formed as b - a, c - a)   out 1: t, or -1 for a miss
 *   fn 1  rayTrianglePair      in 24: origin, direction, (a, e1, e2) of triangle 0, of triangle 1
 *                              out 4: t of each (the raw quotient, also when not accepted), then 1 / 0 per triangle:
 *                              u >= 0, v >= 0, u + v <= 1 (the take adds 0 < t < rec.t)
 *   fn 2  rayTrianglePairP     as fn 1, on the primary-ray record that build_primary_pairs derives for this origin
 *   fn 3  raySphereNear        in 10: origin, direction, centre, radius                           out 1: t, or -1
 *   fn 4  resolve_hit, sphere  in 11: origin, direction, t, centre, radius                        out 7: p, normal, front
 *   fn 5  reflect, refract (eta = iorA / iorB), CalculateReflectance
 *                              in 8: direction, normal, iorA, iorB                                out 7: R, T, reflectProb
 *   fn 6  normalize and the component reciprocals            in 3: v                              out 6: v / |v|, 1 / v
 *   fn 7  one path_shade step (not the last segment, a hit)
 *                              in 33: origin, direction, the Hit's p, normal, t, front (1 / 0), one wcpt_material
 *                              (15 words), the rng state, transmittance
 *                              out 10: the next origin, direction, transmittance, the rng state
 *   fn 8  the child-pair decision of an interior BVH node and the root cull (child_pair, root_survives; the box test has
 *         no fast form, so both modes give the same words)
 *                              in 19: origin, invDirection, the left child's box (min, max), the right child's, rec.t
 *                              out 6: 1 / 0 left child popped first, left box passed, right box passed; the entry
 *                              distance t0 of the left box, of the right box; 1 / 0 the left box as a root survives rec.t */
int      wcpt_selftest_geometry(wcpt_context* ctx, int fn, int arith, const uint32_t* in, uint32_t in_words,
                                uint32_t* out, uint32_t out_words, uint32_t n);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* WCPT_H */
