// Prints the run plan (csrc/run_plan.h) of one shape under given knob values: the header holds no HIP type, so
// tests/test_run_plan.py compiles this with the host compiler under the address and undefined-behaviour sanitizers.
//
//   run_plan_walk model=11 W=2000 H=1000 V=2 patch_size=11 radius_increment=2 fast=1 tex16=1 geom=0 want_strips=0
//                 [ACMMP_KNOB=value ...]    (one command line)
//
// One "name value..." line per plan field; floats as C hexadecimal literals.  The knobs go through read_knobs, with the
// command line in the environment's place.  `run_plan_walk -` takes one such command line per line of standard input
// and ends each plan with a line "end" (the test's matrix in one process).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "run_plan.h"

static int walk(const std::vector<std::string>& args) {
    using namespace acmmp;
    auto arg = [&](const char* name) -> const char* {
        const size_t n = std::strlen(name);
        for (const std::string& a : args)
            if (a.compare(0, n, name) == 0 && a.size() > n && a[n] == '=') return a.c_str() + n + 1;
        return nullptr;
    };
    auto need = [&](const char* name) {
        const char* v = arg(name);
        if (!v) { std::fprintf(stderr, "missing %s\n", name); std::exit(2); }
        return std::atoi(v);
    };
    RunShape sh;
    sh.model = need("model"); sh.W = need("W"); sh.H = need("H"); sh.V = need("V");
    sh.patch_size = need("patch_size"); sh.radius_increment = need("radius_increment");
    sh.fast = need("fast") != 0; sh.tex16 = need("tex16") != 0; sh.geom = need("geom") != 0;
    sh.want_strips = need("want_strips");
    const RunKnobs knobs = read_knobs(arg);
    const RunPlan p = plan_run(sh, knobs);

    std::printf("status %d\n", p.status);
    if (p.status != kPlanOk) {
        std::printf("error %s\n", plan_error(p.status));
        return 0;
    }
    auto num = [](const char* name, long long v) { std::printf("%s %lld\n", name, v); };
    auto real = [](const char* name, float v) { std::printf("%s %a\n", name, static_cast<double>(v)); };
    num("R", p.R); num("nside", p.nside); num("S", p.S); num("Wh", p.Wh); num("rows", p.rows);
    num("Pc", static_cast<long long>(p.Pc));
    num("interp", p.interp); num("ref_interp", p.ref_interp); num("homog", p.homog);
    real("spread_max", p.spread_max); real("neg_tau", p.neg_tau); real("ref_neg_tau", p.ref_neg_tau);
    num("keep", p.keep); num("fix_queue", p.fix_queue); num("ref_fix", p.ref_fix);
    num("ref_split", p.ref_split); num("nb_chunk", p.nb_chunk); num("nb_tile", p.nb_tile);
    num("dead_skip", p.dead_skip); num("ns", p.ns);
    std::string bounds = "bounds", blocks = "ref_blocks", cap = "fix_cap";
    for (int i = 0; i <= p.ns; ++i) bounds += " " + std::to_string(p.bounds[i]);
    for (int i = 0; i < p.ns; ++i) {
        blocks += " " + std::to_string(p.ref_blocks[i]);
        cap += " " + std::to_string(p.fix_cap[i]);
    }
    std::printf("%s\n%s\n%s\n", bounds.c_str(), blocks.c_str(), cap.c_str());
    num("surv_n", static_cast<long long>(p.surv_n)); num("surv_count_n", static_cast<long long>(p.surv_count_n));
    num("surv_pre_n", static_cast<long long>(p.surv_pre_n)); num("psum_n", static_cast<long long>(p.psum_n));
    num("nbfix_n", static_cast<long long>(p.nbfix_n)); num("nbfix_count_n", static_cast<long long>(p.nbfix_count_n));
    num("keep_mask_bytes", 16 * static_cast<long long>(p.psum_n - psum_count(p.Pc, false)));
    num("init_inst", p.init_inst); num("ref_inst", p.ref_inst);
    num("nb_tex", p.nb_tex); num("nb_fm", p.nb_fm); num("nb_masked", p.nb_masked);
    num("sel_mv", p.sel_mv); num("sel_masked", p.sel_masked);
    // the knobs that are no gate
    num("strip_streams", knobs.strip_streams); num("time_all", knobs.time_all);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "-") == 0) {
        for (std::string line; std::getline(std::cin, line);) {
            std::istringstream in(line);
            std::vector<std::string> args;
            for (std::string a; in >> a;) args.push_back(a);
            walk(args);
            std::printf("end\n");
        }
        return 0;
    }
    return walk(std::vector<std::string>(argv + 1, argv + argc));
}
