// hg_device.h — device-side building blocks of the Halogen hot path shared by the kernels of hg_mega.hip
// (lockstep, regenerating and streaming megakernels, and the render server's persistent form of the streaming one;
// their schedulers are hg_sched.h and hg_server.h), the frame blends of hg_blend.hip and the ray queries.
//
// Every function restates a piece of the reference (file:line in its comment) in the reference's
// operation order, compiled with -ffp-contract=off and the shared arithmetic spec include/hg_fmath.h, so the
// results are bit-identical to the CPU oracle.
//
// The code lives in one header per subject, all in namespace hgd; each includes what it uses and compiles alone (make
// headers), so a kernel file may take only the subjects it needs.
#pragma once
#include <hip/hip_runtime.h>

#include "hg_fmath.h"
#include "hg_layout.h"

#pragma clang fp contract(off)

#include "hg_dev_math.h"      // f3, rcp_exact, xform
#include "hg_dev_sampler.h"   // hashes, Sobol closed forms, Sampler
#include "hg_dev_wave.h"      // wave clock, scalar loads, ballots, DPP scans
#include "hg_dev_records.h"   // Ray, Hit, Counters; material, mesh, triangle, node and frame-colour accessors
#include "hg_dev_stack.h"     // Stack, RowVec3/4, RowStack
#include "hg_dev_isect.h"     // boxes, spheres, mesh cull, triangle test, distributed leaf test
#include "hg_dev_trav.h"      // isect_meshes, intersect, the queries' and the resumable traversal
#include "hg_dev_sky.h"       // sample_sky, sky_level
#include "hg_dev_shade.h"     // BSDF, medium stack, trace_ray, camera_ray
