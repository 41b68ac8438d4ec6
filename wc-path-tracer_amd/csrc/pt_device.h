/*
 * pt_device.h — device-side building blocks of the path tracer (gfx950).
 *
 * Semantics follow src/shaders/pathTracer.comp and src/shaders/include/Random.glsl of the reference
 * exactly (cited per function). Every expression keeps the reference's operand order and is compiled
 * with -ffp-contract=off, so that the image is bit-identical to oracle/pt_oracle.c on the same inputs.
 *
 * Layout-level differences from the reference (results unchanged):
 *   - SceneData is a kernel argument (scalar loads from the kernarg segment) instead of a BDA buffer.
 *   - BVH traversal keeps the nearer child in registers and pushes only the farther one, with the box
 *     entry distance t0 on the stack. A child whose box test fails statically (t0 > t1 || t1 < 0) is never
 *     pushed; the dynamic cull (t0 > rt) is applied when the child would have been popped. This is
 *     exactly the reference's pop order and cull set (pathTracer.comp:157-200) with one 64-byte sibling
 *     fetch per interior node instead of 32 (pop) + 64 (children) bytes.
 */
#ifndef WCPT_PT_DEVICE_H
#define WCPT_PT_DEVICE_H

/* The topics, in dependency order; each header includes what it uses and compiles on its own. */
#include "pt_math.h"      /* vector math, exact rcp / sqrt, arithmetic modes */
#include "pt_random.h"    /* PCG, RandomDirection */
#include "pt_geometry.h"  /* rays, nodes, box / sphere / triangle tests, triangle records */
#include "pt_counters.h"  /* counters, RefStack, phase timers, WCPT_DUP_* */
#include "pt_stacks.h"    /* PrivateStack, LdsStack */
#include "pt_traversal.h" /* DrawGeom, the traversal steps, intersect, resolve_hit */
#include "pt_shading.h"   /* CalculateReflectance, PathState, path_shade */
#include "pt_path.h"      /* SplitQueue, TraceTail, TraceRay, primary_direction, store_pixel */

#endif /* WCPT_PT_DEVICE_H */
