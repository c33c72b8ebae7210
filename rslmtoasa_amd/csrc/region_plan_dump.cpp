// region_plan_dump: the region planner of librsrec (region_plan.hpp) as a host-only program, for tests/test_region_plan.py.
//
//   region_plan_dump [--time] PROBLEM      plan the regions of one problem and print the plan (or, with --time, the fastest of five runs in ms)
//   region_plan_dump --match A B           A, B: the seven fields of a RegionKey, comma separated; prints 1 when the keys are equal, else 0
//
// PROBLEM is a text file of white-space separated numbers:
//   kk nslots nmax ntype
//   nb nseed nlev napply two_pass grouped sat_pct
//   keymode                                  0: keys follow, 1: positions follow, 2: keys from the neighbour graph
//   nbr[kk][nslots]                          0-based, -1 absent, slot 0 the atom itself
//   iz0[kk]                                  0-based types
//   key[kk] (keymode 0) | cr[kk][3] (keymode 1)
//   seeds[nb][nseed]                         0-based
// The plan is printed as "name count" lines, each followed by a line of `count` numbers.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "region_plan.hpp"

using namespace rsrec;

namespace {

void put(const char* name, const std::vector<long long>& v) {
    std::printf("%s %zu\n", name, v.size());
    for (long long x : v) std::printf("%lld ", x);
    std::printf("\n");
}
void put(const char* name, const std::vector<int>& v) { put(name, std::vector<long long>(v.begin(), v.end())); }
void put(const char* name, const std::vector<unsigned>& v) { put(name, std::vector<long long>(v.begin(), v.end())); }
void put(const char* name, const std::vector<double>& v) {
    std::printf("%s %zu\n", name, v.size());
    for (double x : v) std::printf("%.17g ", x);
    std::printf("\n");
}

template <class T> bool take(std::istream& in, std::vector<T>& v, size_t n) {
    v.resize(n);
    for (T& x : v) if (!(in >> x)) return false;
    return true;
}

int die(const char* what) { std::fprintf(stderr, "region_plan_dump: %s\n", what); return 2; }

bool parse_key(const char* s, RegionKey& k) {
    int two = 0, grp = 0;
    if (std::sscanf(s, "%d,%d,%d,%d,%d,%d,%d", &k.nb, &k.nseed, &k.nlev, &k.napply, &two, &grp, &k.sat_pct) != 7) return false;
    k.two_pass = two != 0; k.grouped = grp != 0;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "--match")) {
        RegionKey a, b;
        if (!parse_key(argv[2], a) || !parse_key(argv[3], b)) return die("a key is nb,nseed,nlev,napply,two_pass,grouped,sat_pct");
        std::printf("%d\n", a == b ? 1 : 0);
        return 0;
    }
    const bool timed = argc == 3 && !std::strcmp(argv[1], "--time");
    if (argc != 2 && !timed) return die("usage: region_plan_dump [--time] PROBLEM | --match KEY KEY");
    std::ifstream in(argv[argc - 1]);
    if (!in) return die("cannot open the problem file");
    int kk = 0, nslots = 0, nmax = 0, ntype = 0, two = 0, grp = 0, keymode = 0;
    RegionKey key;
    if (!(in >> kk >> nslots >> nmax >> ntype >> key.nb >> key.nseed >> key.nlev >> key.napply >> two >> grp >> key.sat_pct >> keymode)) return die("bad header");
    key.two_pass = two != 0; key.grouped = grp != 0;
    if (kk < 1 || nslots < 1 || nmax < 0 || nmax > kk || ntype < 1 || key.nb < 1 || key.nseed < 1 || key.nlev < 1 || key.napply < 0 || key.sat_pct < 1 || key.sat_pct > 100)
        return die("dimension out of range");
    std::vector<int> nbr, iz0, seeds, radj_ptr, radj;
    std::vector<unsigned> skey;
    std::vector<double> cr;
    if (!take(in, nbr, (size_t)kk * nslots) || !take(in, iz0, kk)) return die("short neighbour table or types");
    for (int n : nbr) if (n < -1 || n >= kk) return die("neighbour outside the lattice");
    for (int t : iz0) if (t < 0 || t >= ntype) return die("type outside 0..ntype-1");
    if (keymode == 0 && !take(in, skey, kk)) return die("short key table");
    if (keymode == 1 && !take(in, cr, (size_t)3 * kk)) return die("short position table");
    if (!take(in, seeds, (size_t)key.nb * key.nseed)) return die("short seed table");
    for (int s : seeds) if (s < 0 || s >= kk) return die("seed outside the lattice");
    reverse_adjacency(kk, nslots, nbr.data(), radj_ptr, radj);
    LatticeView lat{kk, nslots, nmax, ntype, nbr.data(), iz0.data(), radj_ptr.data(), radj.data(), nullptr};
    if (keymode == 1) spatial_key_from_positions(kk, cr.data(), skey);
    if (keymode == 2) spatial_key_from_graph(lat, skey);
    lat.spatial_key = skey.data();

    RegionPlan P;
    double best_ms = 1e300;
    for (int rep = 0; rep < (timed ? 5 : 1); ++rep) {
        P = RegionPlan();
        const auto t0 = std::chrono::steady_clock::now();
        const std::string err = plan_regions(lat, key, seeds.data(), P);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (!err.empty()) return die(err.c_str());
        if (ms < best_ms) best_ms = ms;
    }
    if (timed) { std::printf("%.3f\n", best_ms); return 0; }
    put("key", skey);
    put("order", P.order);
    put("cum", P.cum);
    put("ostride", std::vector<int>{P.ostride});
    put("sat_base", std::vector<int>{P.sat_base});
    put("atom_steps", std::vector<double>{P.atom_steps});
    put("block_mults", std::vector<double>{P.block_mults});
    put("level_max", P.level_max);
    put("hop_min", P.hop_min);
    put("hop_max", P.hop_max);
    put("level_sat", P.level_sat);
    put("level_groups", P.level_groups);
    put("mult_hist", P.mult_hist);
    std::vector<int> runs;
    for (const ClassRun& r : P.sat_runs) { runs.push_back(r.tau); runs.push_back(r.lo); runs.push_back(r.hi); }
    put("sat_runs", runs);
    return 0;
}
