// The library's device translation unit: the C ABI of pt_api.hip, then the image-space passes, side by side.
//
// The passes live in this translation unit because they need the context and the file-local helpers of pt_api.hip (the pointer checks, the
// block compaction of a mask, the drain of the frames in flight).  They add no field to the context and change no line of the frame path:
// pt_api.hip is included as it is, which keeps what was measured on it attached to it (bench.py quotes counter figures only for the kernel
// sources they were collected on).  What a call needs beside the context (counters, a table or two, two events) is allocated per call and
// freed on every exit path by the scaffold of pt_pass.h, outside the timed span.  No pass file includes another (what their kernels share
// is pt_pass_dev.h); a new pass is one more line here (and in the Makefile's PASSES).
#include "pt_api.hip"

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
