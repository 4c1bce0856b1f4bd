// The library's device translation unit, side by side: the frame path of the C ABI (pt_api.hip), the rest of the C ABI by area (pt_subset.hip
// ... pt_multi.hip), then the image-space passes.
//
// Everything lives in this one translation unit because it needs the context and the file-local helpers of pt_api.hip (fail, CK, drain,
// buffer_ptr, bvh_dev), and the passes also those of the area files (the pointer checks of pt_query.hip, the block compaction of
// pt_subset.hip).  Nothing behind pt_api.hip adds a field to the context or changes a line of the frame path: pt_api.hip is included as it
// is, which keeps what was measured on it attached to it (bench.py quotes counter figures only for the kernel sources they were collected
// on, and pt_api.hip is the one file of this list among them).  So new code goes into pt_api.hip only if a default pt_render frame runs
// it; an entry point that a frame does not execute goes into the area file it belongs to, or into a new one: one more line here and in
// the Makefile's AREAS.  The area files stand in the order their text had in pt_api.hip, which is the order in which the template kernels
// of pt_kernels.h are first used.
//
// What a pass needs beside the context (counters, a table or two, two events) is allocated per call and freed on every exit path by the
// scaffold of pt_pass.h, outside the timed span.  No pass file includes another: what their kernels share is pt_pass_dev.h, the scaffold of
// the tiled passes (motion blur, depth of field) included, with its host side in pt_pass.h.  A new pass is one more line here (and in the
// Makefile's PASSES).
#include "pt_api.hip"
#include "pt_subset.hip"
#include "pt_post.hip"
#include "pt_handoff.hip"
#include "pt_query.hip"
#include "pt_views.hip"
#include "pt_inspect.hip"
#include "pt_update.hip"
#include "pt_multi.hip"

#include "pt_pass.h"

#include "pt_gbuffer.hip"
#include "pt_temporal.hip"
#include "pt_filter.hip"
#include "pt_motion.hip"
#include "pt_moments.hip"
#include "pt_plan.hip"
#include "pt_surface.hip"
#include "pt_surface_lod.hip"
#include "pt_upsample.hip"
#include "pt_edge_aa.hip"
#include "pt_exposure.hip"
#include "pt_bloom.hip"
#include "pt_motion_blur.hip"
#include "pt_dof.hip"
#include "pt_lens_warp.hip"
#include "pt_ao.hip"
#include "pt_reflect.hip"
#include "pt_shadow.hip"
