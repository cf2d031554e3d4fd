// Walks the lifetime table of the fusion results (csrc/fusion_results.h) on the host with the class result of
// acmmp_fusion_region_classify held and with the regions as a cause, as fusion.cpp's invalidate does.  Arguments: the
// clouds the mesh, distance, surface, align and class results were computed from (scene, voxels, clean, visible, mesh,
// reference, samples, none).  Prints one line per cause: its name and, for the voxel, clean, visible, mesh, sample,
// render, distance, surface, align and class result, G (gone) or K (kept); then the values of the enumerators that
// must keep theirs, and the cloud each constant of acmmp_fusion_region_classify names.
// test_eval_region_lifetime_table.py reads the lines.  As in fusion_lifetime_walk.cpp the closure is this file's own.
#include <cstdio>
#include <cstring>

#include "fusion_results.h"

using namespace acmmp;

static const char* const kNames[] = {"scene", "voxels", "clean", "visible", "mesh", "reference", "render", "distance",
                                     "surface", "align", "transform", "samples", "classes", "region"};
static const Res kHeld[] = {R_VOXELS, R_CLEAN, R_VISIBLE, R_MESH, R_SAMPLES, R_RENDER, R_DIST, R_SURF, R_ALIGN, R_CLASSES};
static_assert(sizeof(kNames) / sizeof(kNames[0]) == R_REGION + 1, "a name per result");

struct State {
    bool have[R_REGION + 1];
    Res src[R_REGION + 1];
};

static void invalidate(State& s, Res what) {
    for (Res r : kHeld)
        if (s.have[r] && goes_with(r, s.src[r], what)) {
            s.have[r] = false;
            invalidate(s, r);
        }
}

static Res named(const char* name) {
    for (int r = R_SCENE; r <= R_SAMPLES; ++r)
        if (std::strcmp(name, kNames[r]) == 0) return static_cast<Res>(r);
    return R_NONE;
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    for (int cause = R_SCENE; cause <= R_REGION; ++cause) {
        State s;
        for (int r = 0; r <= R_REGION; ++r) { s.have[r] = true; s.src[r] = R_NONE; }
        s.src[R_VOXELS] = R_SCENE;
        s.src[R_CLEAN] = R_VOXELS;
        s.src[R_VISIBLE] = R_CLEAN;
        s.src[R_RENDER] = R_MESH;
        s.src[R_SAMPLES] = R_MESH;
        s.src[R_MESH] = named(argv[1]);
        s.src[R_DIST] = named(argv[2]);
        s.src[R_SURF] = named(argv[3]);
        s.src[R_ALIGN] = named(argv[4]);
        s.src[R_CLASSES] = named(argv[5]);
        invalidate(s, static_cast<Res>(cause));
        std::printf("%s ", kNames[cause]);
        for (Res r : kHeld) std::putchar(s.have[r] ? 'K' : 'G');
        std::putchar('\n');
    }
    std::printf("enumerators %d,%d,%d,%d,%d\n", R_XFORM, R_SAMPLES, R_CLASSES, R_REGION, R_SCENE);
    std::printf("sources ");
    for (int c = 0; c < 8; ++c) {
        const Res r = region_source(c);
        std::printf("%s%s", c ? "," : "", r == R_NONE ? "none" : kNames[r]);
    }
    std::putchar('\n');
    return 0;
}
