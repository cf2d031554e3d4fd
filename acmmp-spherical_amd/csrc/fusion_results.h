// fusion_results.h -- the names of the fusion object's resident results, the one statement of which result goes with
// which (the lifetime paragraphs of include/acmmp.h), and the public source constants as those names.  No HIP type
// appears here, so the table can be compiled and walked on the host alone (tests/fusion_lifetime_walk.cpp).
#pragma once
#include "acmmp.h"

namespace acmmp {

// The resident results.  R_SCENE .. R_REFERENCE and R_SAMPLES are also the clouds a stage can name as its source; R_XFORM
// stands for the cloud transform, which is no result but is replaced like one.  R_SAMPLES comes after R_XFORM: the
// enumerators up to R_XFORM keep their values (tests/fusion_lifetime_walk.cpp indexes its tables by them).
// R_CLASSES is the class result of acmmp_fusion_region_classify; R_REGION stands for the two evaluation regions, which are
// no result but are replaced like one (a set or a clear of either side raises it as the cause).
enum Res { R_NONE = -1, R_SCENE, R_VOXELS, R_CLEAN, R_VISIBLE, R_MESH, R_REFERENCE, R_RENDER, R_DIST, R_SURF, R_ALIGN, R_XFORM,
           R_SAMPLES, R_CLASSES, R_REGION };

// The lifetime table: does the held result `r`, whose record names `src` as the cloud it was computed from, go when
// `cause` has been replaced or discarded?  invalidate (fusion.cpp) applies it transitively, so a row names only the
// direct cause: a mesh of the visible result goes with a voxelize because the visible result does.  src of the voxel,
// the clean, the render and the sample result is always the scene, the voxel, the mesh and the mesh result; src of a mesh that
// acmmp_fusion_set_mesh installed is R_NONE, which is never a cause.  A new stage adds its name above and its row here.
inline bool goes_with(Res r, Res src, Res cause) {
    switch (r) {
        case R_VOXELS: case R_CLEAN: case R_VISIBLE: case R_MESH: case R_RENDER: case R_SAMPLES: return cause == src;
        case R_DIST: return cause == src || cause == R_REFERENCE || cause == R_XFORM || cause == R_REGION;
        case R_ALIGN: return cause == src || cause == R_REFERENCE || cause == R_REGION;
        // with the mesh, with its query cloud, and a reference query's also when the mesh is read in another frame
        case R_SURF: return cause == R_MESH || cause == src || (cause == R_XFORM && src == R_REFERENCE) || cause == R_REGION;
        // the classes of a cloud: with the cloud, with the regions, and a data cloud's with the transform it is read under
        case R_CLASSES: return cause == src || cause == R_REGION || (cause == R_XFORM && src != R_REFERENCE);
        default: return false;                             // the scene and the reference cloud: only replaced
    }
}

// The four families of public source constants as cloud names; R_NONE = no constant of that family.
inline Res vis_source(int s) { return s == ACMMP_VIS_FROM_VOXELS ? R_VOXELS : s == ACMMP_VIS_FROM_CLEAN ? R_CLEAN : R_NONE; }
inline Res mesh_source(int s) {
    return s == ACMMP_MESH_FROM_VOXELS ? R_VOXELS : s == ACMMP_MESH_FROM_CLEAN ? R_CLEAN : s == ACMMP_MESH_FROM_VISIBLE ? R_VISIBLE : R_NONE;
}
inline Res dist_source(int s) {
    switch (s) {
        case ACMMP_DIST_FROM_SCENE: return R_SCENE;
        case ACMMP_DIST_FROM_VOXELS: return R_VOXELS;
        case ACMMP_DIST_FROM_CLEAN: return R_CLEAN;
        case ACMMP_DIST_FROM_VISIBLE: return R_VISIBLE;
        case ACMMP_DIST_FROM_MESH: return R_MESH;
        case ACMMP_DIST_FROM_SAMPLES: return R_SAMPLES;
        default: return R_NONE;
    }
}
// The clouds acmmp_fusion_region_classify takes: a data cloud by its ACMMP_DIST_FROM_* constant, the reference cloud by
// ACMMP_SURF_FROM_REFERENCE.
inline Res region_source(int s) { return s == ACMMP_SURF_FROM_REFERENCE ? R_REFERENCE : dist_source(s); }
inline Res surf_source(int s) {
    switch (s) {
        case ACMMP_SURF_FROM_SCENE: return R_SCENE;
        case ACMMP_SURF_FROM_VOXELS: return R_VOXELS;
        case ACMMP_SURF_FROM_CLEAN: return R_CLEAN;
        case ACMMP_SURF_FROM_VISIBLE: return R_VISIBLE;
        case ACMMP_SURF_FROM_REFERENCE: return R_REFERENCE;
        default: return R_NONE;
    }
}

}  // namespace acmmp
