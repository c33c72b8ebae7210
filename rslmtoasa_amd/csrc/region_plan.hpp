// Host-side planning of the region lists: everything the kernels walk, and every number the launches are sized by, from the neighbour
// table and the seeds of a batch.  Standard library only -- no HIP, no handle: rsrec.hip uploads what plan_regions returns, region_plan_dump.cpp
// prints it.  The region growth of the reference (izero/idum/irlist of hop_b, recursion.f90:1604-1636) is purely topological: one breadth-first
// search (region_levels) gives the level at which every atom joins; "active after L applications of H" = the atoms of levels 0 .. L.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

namespace rsrec {

constexpr int GROUP = 8;            // atoms per wave of the matrix-core kernels (one operator class); the lists are padded into groups of it

// The lattice as the planner reads it (tables of the handle, or of a test).
struct LatticeView {
    int kk, nslots, nmax, ntype;
    const int* nbr;                 // [kk][nslots] 0-based, -1 absent, slot 0 = self
    const int* iz0;                 // 0-based types
    const int *radj_ptr, *radj;     // reverse adjacency: atoms whose neighbour list contains n (reverse_adjacency)
    const unsigned* spatial_key;    // per atom: position along a space-filling curve (locality hint for the order inside a list)
    int op_class(int i) const { return i < nmax ? i : nmax + iz0[i]; }   // per-atom blocks first, then types
};

inline void reverse_adjacency(int kk, int nslots, const int* nbr, std::vector<int>& radj_ptr, std::vector<int>& radj) {
    radj_ptr.assign(kk + 1, 0);
    for (size_t e = 0; e < (size_t)kk * nslots; ++e) if (e % nslots && nbr[e] >= 0) radj_ptr[nbr[e] + 1]++;
    for (int n = 0; n < kk; ++n) radj_ptr[n + 1] += radj_ptr[n];
    radj.resize(radj_ptr[kk]);
    std::vector<int> fill(radj_ptr.begin(), radj_ptr.end() - 1);
    for (size_t e = 0; e < (size_t)kk * nslots; ++e) if (e % nslots && nbr[e] >= 0) radj[fill[nbr[e]]++] = (int)(e / nslots);
}

// The level at which every atom joins the region grown from `seeds`, -1: not within levels 0 .. nlev - 1.  Atom i joins when one of ITS
// neighbour slots holds an atom already inside (the reverse adjacency of the frontier); both_ways: also along the frontier's own slots, which
// makes it the breadth-first distance over the symmetrised neighbour graph.
inline void region_levels(const LatticeView& lat, const int* seeds, int nseed, int nlev, std::vector<int>& dist, bool both_ways = false) {
    dist.assign(lat.kk, -1);
    std::vector<int> frontier, next;
    for (int s = 0; s < nseed; ++s) if (dist[seeds[s]] < 0) { dist[seeds[s]] = 0; frontier.push_back(seeds[s]); }
    for (int level = 0; !frontier.empty() && level + 1 < nlev; ++level) {
        next.clear();
        auto join = [&](int i) { if (i >= 0 && dist[i] < 0) { dist[i] = level + 1; next.push_back(i); } };
        for (int n : frontier) {
            for (int j = 1; both_ways && j < lat.nslots; ++j) join(lat.nbr[(size_t)n * lat.nslots + j]);
            for (int q = lat.radj_ptr[n]; q < lat.radj_ptr[n + 1]; ++q) join(lat.radj[q]);
        }
        frontier.swap(next);
    }
}

struct Region { std::vector<int> dist, order, cum; };   // region_levels of a chain's seeds; atoms by (level, index); cum[L] = #atoms of levels <= L
inline void grow_region(const LatticeView& lat, const int* seeds, int nseed, int nlev, Region& R) {
    region_levels(lat, seeds, nseed, nlev, R.dist);
    R.cum.assign(nlev, 0);
    for (int d : R.dist) if (d >= 0) R.cum[d]++;
    std::vector<int> at(nlev, 0);
    for (int L = 1; L < nlev; ++L) { at[L] = R.cum[L - 1]; R.cum[L] += R.cum[L - 1]; }
    R.order.assign(lat.kk, 0);   // tail is never read (cum bounds every loop)
    for (int i = 0; i < lat.kk; ++i) if (R.dist[i] >= 0) R.order[at[R.dist[i]]++] = i;
}

inline unsigned spread3(unsigned v) {           // 10 bits -> every third bit
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
inline unsigned morton3(unsigned x, unsigned y, unsigned z) { return spread3(x) | (spread3(y) << 1) | (spread3(z) << 2); }

// Locality hint when the caller gives no coordinates: graph distances to three far-apart landmark atoms act as
// pseudo-coordinates (adequate for ordering: atoms with similar distance triples are close in the lattice).
inline void spatial_key_from_graph(const LatticeView& lat, std::vector<unsigned>& key) {
    const int kk = lat.kk;
    std::vector<int> d0, d1, d2;
    int l0 = 0, l1 = 0;
    region_levels(lat, &l0, 1, INT32_MAX, d0, true);
    for (int i = 0; i < kk; ++i) if (d0[i] >= d0[l1]) l1 = i;
    region_levels(lat, &l1, 1, INT32_MAX, d1, true);
    int l2 = 0, best = -1;
    for (int i = 0; i < kk; ++i) { const int m = std::min(d0[i], d1[i]); if (m >= best) { best = m; l2 = i; } }
    region_levels(lat, &l2, 1, INT32_MAX, d2, true);
    key.resize(kk);
    for (int i = 0; i < kk; ++i) key[i] = morton3((unsigned)std::max(d0[i], 0), (unsigned)std::max(d1[i], 0), (unsigned)std::max(d2[i], 0));
}

// With coordinates cr[kk][3]: the Morton code of the position, 10 bits per axis over the largest span.
inline void spatial_key_from_positions(int kk, const double* cr, std::vector<unsigned>& key) {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int i = 0; i < kk; ++i)
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], cr[3 * (size_t)i + a]); hi[a] = std::max(hi[a], cr[3 * (size_t)i + a]); }
    double span = 1e-300;
    for (int a = 0; a < 3; ++a) span = std::max(span, hi[a] - lo[a]);
    key.resize(kk);
    for (int i = 0; i < kk; ++i) {
        unsigned q[3];
        for (int a = 0; a < 3; ++a) q[a] = (unsigned)std::min(1023.0, std::max(0.0, (cr[3 * (size_t)i + a] - lo[a]) / span * 1023.0));
        key[i] = morton3(q[0], q[1], q[2]);
    }
}

// What a plan depends on besides the lattice and the seeds [nb][nseed]: chains, seeds per chain, levels of the lists, applications of H per
// chain; two passes (levels) per application (hoh); lists padded into operator-class groups of GROUP (matrix-core kernels); the share of
// the lattice (per cent) from which a chain's region runs on the list of ALL atoms.
struct RegionKey {
    int nb = 0, nseed = 0, nlev = 0, napply = 0;
    bool two_pass = false, grouped = false;
    int sat_pct = 100;
    bool operator==(const RegionKey& o) const {
        return nb == o.nb && nseed == o.nseed && nlev == o.nlev && napply == o.napply && two_pass == o.two_pass && grouped == o.grouped && sat_pct == o.sat_pct;
    }
};
struct ClassRun { int tau, lo, hi; };   // groups lo .. hi - 1 of the list of all atoms hold operator class tau

// What the host keeps of a plan once the lists are on the device.
struct RegionStats {
    int ostride = 0, sat_base = 0;      // entries of one chain's order row; offset of the list of all atoms inside it
    double atom_steps = 0, block_mults = 0;
    std::vector<int> level_max;         // per level: largest count of either list over the chains (sizes the launches)
    std::vector<int> hop_min, hop_max;  // per level: smallest / largest count of the H|psi> lists (padding included) over the chains
    std::vector<double> level_groups;   // [level][tau]: groups of 8 atoms (padding included) of operator class tau, summed over the chains
    std::vector<double> mult_hist;      // [pass 0/1][tau][nslots + 1]: block multiplications of the call by (pass, operator class, slot), summed over the chains
    std::vector<ClassRun> sat_runs;     // the list of ALL atoms is sorted by operator class: one run of groups per class
    std::vector<int> level_sat;         // per level: chains that use that list
};
struct RegionPlan : RegionStats {
    std::vector<int> order;             // [nb][ostride], see plan_regions
    std::vector<int> cum;               // [nb][nlev] counts, [nb][nlev] list offsets (the lists of H|psi>), then the same two tables for the streaming passes
};

// The order inside every list: operator class first (groups must be homogeneous), then position.
struct ListOrder {
    const LatticeView& lat;
    bool grouped;
    int cls(int i) const { return grouped ? lat.op_class(i) : 0; }
    bool operator()(int x, int y) const {
        const int tx = cls(x), ty = cls(y);
        if (tx != ty) return tx < ty;
        if (lat.spatial_key[x] != lat.spatial_key[y]) return lat.spatial_key[x] < lat.spatial_key[y];
        return x < y;
    }
};

// Appends the sorted `atoms` to a row at w; grouped: every class run padded with -1 to a multiple of GROUP.  G: the groups begun, by class.
inline void append_list(const ListOrder& ord, const int* atoms, size_t n, int* row, int& w, double* G = nullptr) {
    for (size_t q = 0; q < n; ++q) {
        if (ord.grouped && q > 0 && ord.cls(atoms[q]) != ord.cls(atoms[q - 1])) while (w % GROUP) row[w++] = -1;
        if (G && w % GROUP == 0) G[ord.cls(atoms[q])] += 1.0;
        row[w++] = atoms[q];
    }
    if (ord.grouped) while (w % GROUP) row[w++] = -1;
}

// The list of all atoms: the same for every chain of the lattice.
inline std::vector<int> all_atoms_list(const ListOrder& ord, int cap) {
    std::vector<int> all(ord.lat.kk), list(cap, -1);
    std::iota(all.begin(), all.end(), 0);
    std::sort(all.begin(), all.end(), ord);
    int n = 0;
    append_list(ord, all.data(), all.size(), list.data(), n);
    list.resize(n);
    return list;
}

// One chain's lists (orow = [level-major | per level from cap_pre | all atoms at sat_off]) and its rows of the four `cum` tables (crow, `tab`
// entries apart).  Regions of sat_from atoms run on the list of all atoms.  G [nlev][ntau]: groups of every level's own H|psi> list.
inline void chain_lists(const ListOrder& ord, const Region& R, const std::vector<int>& sat_list, int cap_pre, int sat_off, int sat_from, int nlev, int* orow, int* crow,
                        size_t tab, double* G, int ntau) {
    int *brow = crow + tab, *crow2 = crow + 2 * tab, *brow2 = crow + 3 * tab;
    std::copy(sat_list.begin(), sat_list.end(), orow + sat_off);
    int w = cap_pre, wp = 0;
    std::vector<int> lev, region, merged;
    for (int L = 0; L < nlev; ++L) {
        const int lo = L ? R.cum[L - 1] : 0, hi = R.cum[L];
        // once the region covers most of the lattice the sorted list of all atoms is used instead: blocks outside
        // the region are exactly zero, so a superset changes nothing
        if (hi >= sat_from) { crow[L] = crow2[L] = (int)sat_list.size(); brow[L] = brow2[L] = sat_off; continue; }
        lev.assign(R.order.begin() + lo, R.order.begin() + hi);
        std::sort(lev.begin(), lev.end(), ord);
        append_list(ord, lev.data(), lev.size(), orow, wp);              // level-major list: this shell behind the earlier ones
        crow2[L] = wp; brow2[L] = 0;
        if (L > 0 && hi == lo) { crow[L] = crow[L - 1]; brow[L] = brow[L - 1]; continue; }     // the region has stopped growing: the previous level's list again
        merged.resize(region.size() + lev.size());
        std::merge(region.begin(), region.end(), lev.begin(), lev.end(), merged.begin(), ord);
        region.swap(merged);
        brow[L] = w;
        append_list(ord, region.data(), region.size(), orow, w, G + (size_t)L * ntau);
        crow[L] = w - brow[L];
    }
}

// One chain's bookkeeping in the reference's terms: application t (1..napply) multiplies one block per (atom, slot) whose source atom lies
// in the region before it.  H [2][ntau][nslots + 1]: the multiplications by (pass, operator class of the target, slot), added up over the
// chains -- the reference's count is their sum, the flops the block structure requires weigh them by block class.
inline void chain_counts(const LatticeView& lat, const RegionKey& K, const std::vector<int>& lev_of, double* H) {
    const int ns = lat.nslots, nfs = ns + 1, ntau = lat.nmax + lat.ntype;
    // uses1(d) / uses2(d): applications t whose first / second (hoh) pass sees a source at distance d inside the region -- d <= t - 1; with two
    // passes d <= 2 (t - 1) / d <= 2 t - 1
    auto uses1 = [&](int d) { return (double)std::max(0, K.napply - (K.two_pass ? (d + 1) / 2 : d)); };
    auto uses2 = [&](int d) { return (double)std::max(0, K.napply - d / 2); };
    // one multiplication per (target atom i, slot s) whose source nbr(i, s) is active (hop_b :1576-1625)
    for (int i = 0; i < lat.kk; ++i) {
        const int ti = lat.op_class(i);
        for (int s = 0; s < ns; ++s) {
            const int n = lat.nbr[(size_t)i * ns + s];
            if (n < 0 || lev_of[n] < 0) continue;
            H[(size_t)ti * nfs + s] += uses1(lev_of[n]);
            if (K.two_pass) H[((size_t)ntau + ti) * nfs + s] += uses2(lev_of[n]);
        }
        if (K.two_pass && lev_of[i] >= 0) H[((size_t)ntau + ti) * nfs + ns] += uses1(lev_of[i]);   // e_nu psi + l.s psi on-site (:1437-1438), one merged block here
    }
}

// The per-level statistics of a finished plan.  lgroups [chain][level][tau]: chain_lists' G.
inline void level_statistics(const LatticeView& lat, const RegionKey& K, const std::vector<int>& sat_list, const std::vector<double>& lgroups, RegionPlan& P) {
    const int nb = K.nb, nlev = K.nlev, ntau = lat.nmax + lat.ntype, sat_groups = (int)sat_list.size() / GROUP;
    P.level_max.assign(nlev, 0); P.hop_min.assign(nlev, INT32_MAX); P.hop_max.assign(nlev, 0); P.level_sat.assign(nlev, 0);
    P.level_groups.assign((size_t)nlev * ntau, 0.0);
    // groups by operator class: the saturated list is the same for every chain; a level-major list is walked once per chain
    std::vector<double> sat_hist(ntau, 0.0);
    for (int g = 0; g < sat_groups; ++g) {
        const int t = lat.op_class(sat_list[(size_t)g * GROUP]);
        sat_hist[t] += 1.0;
        if (!K.grouped) continue;
        if (P.sat_runs.empty() || P.sat_runs.back().tau != t) P.sat_runs.push_back({t, g, g + 1});
        else P.sat_runs.back().hi = g + 1;
    }
    const int *cnt = P.cum.data(), *off = cnt + (size_t)nb * nlev, *cnt2 = off + (size_t)nb * nlev;
    for (int c = 0; c < nb; ++c) {
        const double* prev = nullptr;
        for (int l = 0; l < nlev; ++l) {
            const size_t cl = (size_t)c * nlev + l;
            P.level_max[l] = std::max({P.level_max[l], cnt[cl], cnt2[cl]});   // (the larger of the two lists' counts sizes the launches)
            P.hop_min[l] = std::min(P.hop_min[l], cnt[cl]); P.hop_max[l] = std::max(P.hop_max[l], cnt[cl]);
            const bool sat = off[cl] == P.sat_base;       // (the chain is on the list of all atoms)
            P.level_sat[l] += sat;
            const double* G = lgroups.data() + cl * ntau;
            if (!sat && l > 0 && off[cl] == off[cl - 1] && prev) G = prev;     // the previous level's list again
            for (int t2 = 0; t2 < ntau; ++t2) P.level_groups[(size_t)l * ntau + t2] += sat ? sat_hist[t2] : G[t2];
            prev = sat ? nullptr : G;
        }
    }
}

// One task per chain on a few short-lived host threads.  (Not OpenMP: its idle workers spin for 200 ms after a
// parallel region -- one per visible CPU, 256 on the GPU boxes -- and burn the process's CPU quota: the host thread was then
// descheduled for 60-90 ms at a time during the next two or three calls, inside whatever HIP call it happened to be in.)
template <class F> void for_each_chain(int nb, F&& fn) {
    const int nthr = std::max(1, std::min({nb, 8, (int)std::thread::hardware_concurrency()}));
    if (nthr == 1) { for (int c = 0; c < nb; ++c) fn(c); return; }
    std::atomic<int> next_chain{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < nthr; ++t)
        pool.emplace_back([&]() { for (int c = next_chain++; c < nb; c = next_chain++) fn(c); });
    for (auto& th : pool) th.join();
}

// The regions of one batch.  seeds0: [nb][nseed] 0-based.  Returns an error text, empty when the plan stands.
// order row = [level-major | per level | all atoms].  grouped: every list is sorted by operator class (per-atom blocks first, then types) and
// each class run is padded with -1 to a multiple of GROUP, so that 8 consecutive entries always share their operator blocks (MFMA kernels).
// H|psi> gathers: it walks one list per level of the growing region, position-sorted as a whole (the locality of the list of all atoms).  The
// streaming passes behind it read every active block once and gather nothing: they keep the level-major list (shell after shell; a level = a
// prefix), whose walk is closer to address order.  Measurements of both: DESIGN section 3.
inline std::string plan_regions(const LatticeView& lat, const RegionKey& K, const int* seeds0, RegionPlan& P) {
    const int kk = lat.kk, nb = K.nb, nlev = K.nlev, ntau = lat.nmax + lat.ntype;
    const int cap = K.grouped ? kk + 7 * lat.nmax + 7 * lat.ntype + 8 : kk;          // capacity of one list of all atoms
    const int cap_pre = ((K.grouped ? kk + 7 * lat.nmax + 7 * lat.ntype * nlev + 8 : kk) + GROUP - 1) / GROUP * GROUP;   // capacity of the level-major list (a multiple of 8: every list starts on a group border)
    const int sat_from = (int)(((long)K.sat_pct * kk + 99) / 100);   // regions of at least this many atoms run on the list of all atoms (100: only the whole lattice)
    // the regions first, then the row size they need
    std::vector<Region> regs(nb);
    for_each_chain(nb, [&](int c) { grow_region(lat, seeds0 + (size_t)c * K.nseed, K.nseed, nlev, regs[c]); });
    size_t lvneed = 8;
    for (int c = 0; c < nb; ++c) {
        size_t need = 0;
        for (int L = 0; L < nlev; ++L) {
            const int n = regs[c].cum[L];
            if (n >= sat_from || (L > 0 && n == regs[c].cum[L - 1])) continue;       // list of all atoms / the previous level's list again
            need += (size_t)n + (K.grouped ? (size_t)7 * std::min(ntau, n) + 8 : 0);
        }
        lvneed = std::max(lvneed, need);
    }
    lvneed = (lvneed + 7) / 8 * 8;
    for (const size_t entries : {lvneed + (size_t)cap, (size_t)cap_pre + lvneed + (size_t)cap})
        if (entries > (size_t)INT32_MAX) {
            char text[96];
            std::snprintf(text, sizeof text, "region lists of %zu entries per chain exceed the index range", entries);
            return text;
        }
    P.sat_base = cap_pre + (int)lvneed; P.ostride = P.sat_base + cap;
    P.order.assign((size_t)nb * P.ostride, -1); P.cum.assign((size_t)4 * nb * nlev, 0);
    const ListOrder ord{lat, K.grouped};
    const std::vector<int> sat_list = all_atoms_list(ord, cap);
    const size_t hist_n = (size_t)2 * ntau * (lat.nslots + 1);
    std::vector<double> hist((size_t)nb * hist_n, 0.0), lgroups((size_t)nb * nlev * ntau, 0.0);
    for_each_chain(nb, [&](int c) {
        chain_lists(ord, regs[c], sat_list, cap_pre, P.sat_base, sat_from, nlev, P.order.data() + (size_t)c * P.ostride, P.cum.data() + (size_t)c * nlev,
                    (size_t)nb * nlev, lgroups.data() + (size_t)c * nlev * ntau, ntau);
        chain_counts(lat, K, regs[c].dist, hist.data() + (size_t)c * hist_n);
    });
    P.mult_hist.assign(hist_n, 0.0);
    for (int c = 0; c < nb; ++c) {
        for (int t = 1; t <= K.napply; ++t) P.atom_steps += regs[c].cum[std::min(K.two_pass ? 2 * t : t, nlev - 1)];   // post-hop work runs on the region after the application
        for (size_t q = 0; q < hist_n; ++q) P.mult_hist[q] += hist[(size_t)c * hist_n + q];
    }
    for (size_t q = 0; q < hist_n; ++q) P.block_mults += P.mult_hist[q];   // (whole numbers: exact in any order)
    if (K.two_pass) for (size_t q = hist_n / 2 + lat.nslots; q < hist_n; q += lat.nslots + 1) P.block_mults += P.mult_hist[q];   // the reference multiplies enim and lsham separately
    level_statistics(lat, K, sat_list, lgroups, P);
    return std::string();
}

}  // namespace rsrec
