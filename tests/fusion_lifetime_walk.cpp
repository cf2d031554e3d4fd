// Walks the lifetime table of the fusion results (csrc/fusion_results.h) on the host, as fusion.cpp's invalidate does.
// Arguments: the clouds the visible, mesh, distance, surface and align results were computed from (scene, voxels,
// clean, visible, mesh, reference, none).  Prints one line per cause: its name and, for the voxel, clean, visible,
// mesh, render, distance, surface and align result, G (gone) or K (kept).  test_fusion_lifetime_table.py compares the
// lines with the matrix of test_gpu_fusion_lifetimes.py.
// The closure below is this file's own, over its own list of held results: it checks goes_with and the source maps'
// names against the matrix, not fusion.cpp's invalidate.  A record missing from invalidate's drop lines shows only in
// test_gpu_fusion_lifetimes.py.
#include <cstdio>
#include <cstring>

#include "fusion_results.h"

using namespace acmmp;

static const char* const kNames[] = {"scene", "voxels", "clean", "visible", "mesh", "reference", "render", "distance",
                                     "surface", "align", "transform"};
static const Res kHeld[] = {R_VOXELS, R_CLEAN, R_VISIBLE, R_MESH, R_RENDER, R_DIST, R_SURF, R_ALIGN};

struct State {
    bool have[R_XFORM + 1];
    Res src[R_XFORM + 1];
};

static void invalidate(State& s, Res what) {
    for (Res r : kHeld)
        if (s.have[r] && goes_with(r, s.src[r], what)) {
            s.have[r] = false;
            invalidate(s, r);
        }
}

static Res named(const char* name) {
    for (int r = R_SCENE; r <= R_REFERENCE; ++r)
        if (std::strcmp(name, kNames[r]) == 0) return static_cast<Res>(r);
    return R_NONE;
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    for (int cause = R_SCENE; cause <= R_XFORM; ++cause) {
        State s;
        for (int r = 0; r <= R_XFORM; ++r) { s.have[r] = true; s.src[r] = R_NONE; }
        s.src[R_VOXELS] = R_SCENE;
        s.src[R_CLEAN] = R_VOXELS;
        s.src[R_RENDER] = R_MESH;
        s.src[R_VISIBLE] = named(argv[1]);
        s.src[R_MESH] = named(argv[2]);
        s.src[R_DIST] = named(argv[3]);
        s.src[R_SURF] = named(argv[4]);
        s.src[R_ALIGN] = named(argv[5]);
        invalidate(s, static_cast<Res>(cause));
        std::printf("%s ", kNames[cause]);
        for (Res r : kHeld) std::putchar(s.have[r] ? 'K' : 'G');
        std::putchar('\n');
    }
    return 0;
}
