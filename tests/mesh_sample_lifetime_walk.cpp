// Walks the lifetime table of the fusion results (csrc/fusion_results.h) on the host with the sample result held, as
// fusion.cpp's invalidate does.  Arguments: the clouds the mesh, distance, surface and align results were computed from
// (scene, voxels, clean, visible, mesh, reference, samples, none).  Prints one line per cause: its name and, for the
// voxel, clean, visible, mesh, sample, render, distance, surface and align result, G (gone) or K (kept); then the
// ACMMP_DIST_FROM_* constant whose cloud is the sample result.  test_mesh_sample_lifetime_table.py reads the lines.
// As in fusion_lifetime_walk.cpp the closure is this file's own, over its own list of held results.
#include <cstdio>
#include <cstring>

#include "fusion_results.h"

using namespace acmmp;

static const char* const kNames[] = {"scene", "voxels", "clean", "visible", "mesh", "reference", "render", "distance",
                                     "surface", "align", "transform", "samples"};
static const Res kHeld[] = {R_VOXELS, R_CLEAN, R_VISIBLE, R_MESH, R_SAMPLES, R_RENDER, R_DIST, R_SURF, R_ALIGN};
static_assert(sizeof(kNames) / sizeof(kNames[0]) == R_SAMPLES + 1, "a name per result");

struct State {
    bool have[R_SAMPLES + 1];
    Res src[R_SAMPLES + 1];
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
    if (argc != 5) return 2;
    for (int cause = R_SCENE; cause <= R_SAMPLES; ++cause) {
        State s;
        for (int r = 0; r <= R_SAMPLES; ++r) { s.have[r] = true; s.src[r] = R_NONE; }
        s.src[R_VOXELS] = R_SCENE;
        s.src[R_CLEAN] = R_VOXELS;
        s.src[R_VISIBLE] = R_CLEAN;
        s.src[R_RENDER] = R_MESH;
        s.src[R_SAMPLES] = R_MESH;
        s.src[R_MESH] = named(argv[1]);
        s.src[R_DIST] = named(argv[2]);
        s.src[R_SURF] = named(argv[3]);
        s.src[R_ALIGN] = named(argv[4]);
        invalidate(s, static_cast<Res>(cause));
        std::printf("%s ", kNames[cause]);
        for (Res r : kHeld) std::putchar(s.have[r] ? 'K' : 'G');
        std::putchar('\n');
    }
    for (int c = 0; c < 16; ++c)
        if (dist_source(c) == R_SAMPLES) std::printf("constant %d\n", c);
    std::printf("surface_source %s\n", surf_source(ACMMP_DIST_FROM_SAMPLES) == R_SAMPLES ? "samples" : "other");
    return 0;
}
