// Stand-in for "Maths.h", used only by oracle/ref_build/ref_disney.cpp and ref_device.cpp (test infrastructure).
// HelloPathtracing_original/Material.h says #include "Maths.h".  The reference builds on Windows, whose
// include lookup ignores letter case, so there the name finds maths.h beside Material.h.  On a
// case-sensitive file system it would find OptixUtils/Maths.h instead, whose second sqr() makes the
// call in Disney.cuh's Fr ambiguous.  This file restores the Windows lookup; it declares nothing.
#pragma once
#include "maths.h"
