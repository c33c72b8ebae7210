// librsrec: C ABI (include/rsrec.h) + host orchestration of the MI355X recursion engine.
//
// Reference path replaced: source/recursion.f90 of rslmtoasa/rslmtoasa -- recur_b/crecal_b/hop_b/hop_b_hoh
// (:1807/:1873/:1560/:1411), chebyshev_recur & helpers (:3057, :2145-2763), recur/crecal/hop (:3485/:3423/:3310),
// zsqr (:1980).  Everything numerical runs in hand-written HIP kernels for gfx950; there is no CPU fallback.
//
// Engine design:
//  * all chains of a call are independent (one per recursion site); they are advanced TOGETHER in batches so that
//    the small active regions of the first steps still fill the 256 CUs;
//  * the region growth of the reference (izero/idum/irlist) is purely topological: a breadth-first search from the
//    seed on the host gives the atom order; "active after L applications of H" = a prefix of that order;
//  * work vectors (psi, pmn, ...) never leave HBM; only the 18x18 coefficients come back to the host;
//  * reductions are two-stage and fixed-order (no float atomics) so results are run-to-run reproducible.
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <dlfcn.h>
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/rsrec.h"
#include "region_plan.hpp"
#include "kernels_valu.hpp"
#include "kernels_mfma.hpp"
#include "kernels_spmm4.hpp"
#include "kernels_spmm5.hpp"
#include "kernels_uscheme.hpp"
#include "kernels_green.hpp"
#include "kernels_ldos.hpp"
#include "kernels_spectra.hpp"
#include "kernels_moments.hpp"
#include "kernels_kubo.hpp"
#include "kernels_cond.hpp"
#include "kernels_optical.hpp"
#include "kernels_exchange.hpp"
#include "kernels_auxgreen.hpp"
#include "kernels_contour.hpp"
#include "kernels_assemble.hpp"
#include "kernels_fan.hpp"
#include "kernels_bloch.hpp"
#include "kernels_blochmap.hpp"
#include "kernels_lattice.hpp"
#include "kernels_shot.hpp"
#include "kernels_sitemap.hpp"
#include "kernels_evolve.hpp"

using namespace rsrec;

namespace {

// Owned device memory: freed when the owner goes (the handle, a region entry); moves, never copies.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n) {
        if (n <= bytes) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

}  // namespace

struct rsrec_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;     // device -> host copies of the Green stage, overlapped with its kernels
    hipEvent_t ev_green[2] = {nullptr, nullptr};
    hipStream_t side_stream = nullptr;     // B_{n+1} reduction + eigen-solve of level n, concurrent with H u_{n+1} of level n + 1 (u-scheme)
    hipEvent_t ev_orth = nullptr, ev_bred = nullptr;
    hipStream_t oct_stream = nullptr;      // the chain-octet launch of a level's H|psi> beside its main launch (disjoint outputs)
    hipEvent_t ev_oct_in = nullptr, ev_oct_out = nullptr;
    size_t p2_slot = 0;                    // doubles per slot of d_partial2 (slot 1: the side stream's presum)
    std::string err;
    // lattice (host copies for the region search + device tables)
    bool have_lattice = false, have_ham = false;
    std::vector<int32_t> lat_nn, lat_iz;   // the caller's tables as last uploaded: an SCF loop passes the same lattice every iteration
    int lat_nncols = 0;
    std::vector<double> lat_cr;
    int kk = 0, nslots = 0, nmax = 0, ntype = 0;
    std::vector<int> nbr;        // [kk][nslots] 0-based, -1 absent, slot 0 = self
    std::vector<int> iz0;        // 0-based types
    std::vector<int> radj_ptr, radj;  // reverse adjacency: atoms whose neighbour list contains n
    DevBuf d_nbr, d_iz, d_nbr5;   // nbr5: (kk+1) x (nslots+2), absent neighbours and the extra row point at the zero block (k_spmm5)
    // hamiltonian
    int hslots = 0, hoh = 0, nsp = 2;
    DevBuf d_hst, d_hloc, d_host, d_holoc, d_enim, d_lsham;
    Spmm4Operator s4_op;
    int s4_built_split = 0;
    Spmm5Operator s5_op;
    DevBuf d_s5queue;            // group counters of the persistent k_spmm5 form
    int s5_built = 0;
    size_t s5_lds_limit = (size_t)-1;   // LDS a k_spmm5 workgroup may ask for on THIS handle's device ((size_t)-1: not asked yet; hipFuncSetAttribute is per device)
    int n_cu = 0;                       // compute units of the device (size of the persistent launches)
    bool s4_attr = false;               // k_spmm4's LDS opt-in, per handle for the same reason
    // dynamic LDS granted on this handle to k_terminator, k_chebyshev_ldos and k_chebyshev_spectra (lds_opt_in; the 64 KB every kernel may
    // have need no asking, and k_terminator has always asked)
    size_t term_lds = 0, cheb_ldos_lds = (size_t)64 * 1024, cheb_spec_lds = (size_t)64 * 1024;
    std::vector<double> host_ee, host_lsham, host_eeo, host_enim, host_hall, host_hallo;   // operator arrays as last set (Kubo operator tables; local-axis runs)
    std::vector<double> host_st, host_loc;   // ee / hall with l.s folded into the on-site block when !hoh (what d_hst / d_hloc hold)
    // raw blocks assembled on the device (rsrec_assemble_blocks): [part: 0 per-type, 1 per-atom][0: blocks, 1: blocks x obar]; asm_host = what the
    // caller got back -- rsrec_set_hamiltonian recognises those arrays bitwise and then takes the device copies instead of uploading
    DevBuf d_asm[2][2], d_asm_in;
    std::vector<double> asm_host[2][2];
    int asm_nslots[2] = {0, 0}, asm_ncls[2] = {0, 0}, asm_hoh[2] = {0, 0};
    int n_octet_launch = 0;      // launches of the last call that formed the groups of per-atom-block atoms over 8 chains (k_spmm5<., false, true>)
    int n_asm_reused = 0;        // block arrays the last rsrec_set_hamiltonian took from those device copies (0..4)
    long n_asm_calls = 0, n_ldos_calls = 0, n_recursion_calls = 0;   // life-time counters of the handle (RSREC_REPORT)
    Spmm5Operator s5_la; int s5_la_ok = 0;   // operator tables of local-axis runs: H without the on-site l.s term, which comes per chain
    DevBuf d_la_extra, d_rot;               // per-chain on-site fragments; the rotations of all chains of the call (k_rotate_coef)
    Spmm5Operator kubo_op[RSREC_KUBO_NOUT_MAX], kubo_op_b[RSREC_KUBO_NIN_MAX], kubo_hbulk;   // output operators (v_a: [0]) / input operators (v_b: [0]) of the last rsrec_kubo_moments call
    Spmm5Operator orb_plain;                // h as ham_vec_matmul applies it when hoh is set (rsrec_orbital_moments, rsrec_apply_operator vel = 2)
    // work
    DevBuf d_green_in, d_green_out;   // inputs and outputs of the calls on caller arrays: the Green stages (green_pipeline), rsrec_terminator,
                                      // rsrec_scalar_density, and the pair calls (PairCall)
    DevBuf d_kubo[5];                 // rsrec_kubo_moments: work vectors, left / right matrices, slice partials, moments -- kept between calls (tens of GB:
                                      // their hipMalloc / hipFree cost 0.1-1.3 s per call on some boxes of the pool); given back when the recursion plans a batch
    DevBuf d_cond[4];                 // rsrec_kubo_integrand: basis tables, S / D planes, column-tile partials, staging (mu diagonals, integrand);
                                      // given back with d_kubo when the recursion plans a batch
    DevBuf d_ctens[2];                // rsrec_kubo_conductivity: mesh + series as k_cond_tensor reads them; staging (integrand in, sigma / series out);
                                      // given back with d_cond
    DevBuf d_opt[5];                  // rsrec_kubo_optical: tables (basis, Fermi weights and ranges, live tiles); moment planes, projections and tile
                                      // partials of a chunk of orbitals; staging (a set's diagonals in, opt out); given back with d_cond
    DevBuf d_bsqrt, d_term, d_gim, d_ldos;   // stages on resident coefficients: sqrt(B^2), terminators; LDOS stage: Im g0_jj, output images
    DevBuf d_ops, d_spec;                    // spectra stage: operators (+ their traces with the Chebyshev moments), Im Tr(O g0) of the rank's sites
    // the image the last spectra call left in d_spec ([site][nen][nop] of the rank's sites), for rsrec_spectra_integrals(spec = NULL):
    // nop = 0: none.  Dropped where the resident chains are dropped.
    struct SpecImage { int nop = 0, nen = 0, n = 0, site_offset = 0, nsites_total = 0; } spec_res;
    DevBuf d_mint;                           // rsrec_spectra_integrals: uploaded inputs | series | running sums | mesh | output images
    void* pin = nullptr;              // pinned host staging buffer: every per-call transfer goes through it (see xfer_*)
    size_t pin_bytes = 0;
    DevBuf d_frags, d_vec[6], d_partial, d_partial2, d_coefA, d_coefB, d_bmats, d_status, d_seed, d_seedcoef, d_mu, d_scal, d_zsqr;
    DevBuf d_fan, d_fan_tab, d_mpair;   // rsrec_chebyshev_pairs_direct: gathered blocks M(18,18,nmom,entry); entry and pair tables; M_ij / M_ji of every pair
    DevBuf d_bloch_geo, d_bloch_tab;    // rsrec_chebyshev_bloch: positions and k-points of the call; lists, segment offsets and level counts of a batch
    DevBuf d_map_w;                     // rsrec_chebyshev_bloch_map: the weights w(n, e) of the call
    DevBuf d_shot_w;                    // rsrec_kubo_single_shot: the weights of the call, [conj(wl) | wr][e][order]
    DevBuf d_evo_w;                     // rsrec_chebyshev_evolve: the step's weights w(order) of the call
    DevBuf d_site_w, d_site_coef;       // rsrec_chebyshev_site_map: the weights w(n, e) of the call; the conjugated coefficient tables of a batch, (kk) per vector
    DevBuf d_lat_tab, d_lat_w, d_lat_part;   // rsrec_chebyshev_lattice: lists and offsets of a batch; weights and divergence bounds; split partials
    // options
    long opt_batch = 0, opt_kernels = 0, opt_nblk = 0, opt_spmm5 = 2, opt_chain_fold = 1, opt_s5_cap = 0, opt_side = 1, opt_s5_lds = 1, opt_s5_queue = 1, opt_cheb_fused = 1;
    long opt_s5_waves = 8;
    long opt_sat_pct = 100;      // a chain whose region holds at least this share (per cent) of the lattice runs on the list of ALL atoms (blocks outside the region are zero); rounds 1-3: 80 -- with a position-sorted list per level the superset no longer buys locality and costs its extra atoms (46^3: -1 %)
    long opt_orth_oop = 1;       // 1 = k_mfma_orth3 writes u_{n+1} into a third u vector instead of over u_{n-1} (faster on the HBM; one more work vector)
    long opt_s5_split = 0;       // persistent k_spmm5: 3 = a wave takes a third of a group's tiles (k_spmm5<., true, false, 3>; s5_waves = 8 .. 12 waves per CU then, clamped to the 768 threads of its launch bounds)
    long opt_s5_run_min = 0;     // operators with several classes: smallest class run (in groups) that gets an LDS launch of its own (0: by launch size)
    long opt_s5_spin_xcd = 0;    // persistent k_spmm5 on collinear operators: 1 = even XCDs serve output spin 0, odd XCDs spin 1; 0 = both spins on every XCD
    long opt_s5_octet = 8;       // atoms with their own operator blocks (nmax) from which their groups are formed over 8 CHAINS instead of one atom + 7 padding tiles (0: never; round 3: 64; B2FeCo, nmax = 15: 2.38 -> 2.34 ms per launch)
    long opt_s5_host_emit = 0;   // 1: swizzle k_spmm5's operator streams on the host (round-2 path) instead of assembling them on the device
    long opt_kubo_lchunk = 0;    // rsrec_kubo_moments: left vectors held at a time (0: as many as fit)
    long opt_kubo_vbatch = 0;    // rsrec_kubo_moments: random vectors advanced together as the chains of one launch (0: up to 8, as many as fit beside a whole left matrix)
    long opt_lattice_vbatch = 0; // rsrec_chebyshev_lattice: chains advanced together as the chains of one launch (0: up to 8, as many as fit)
    long opt_blochmap_orders = 2;  // rsrec_chebyshev_bloch_map: orders added to the accumulators per pass (1 | 2: same bits, see kernels_blochmap.hpp)
    long opt_blochmap_kchunk = 0;  // rsrec_chebyshev_bloch_map: k-points per chunk of the final sums (0: 256, one launch's rows of the phase matrix); tests force it small
    long opt_shot_orders = 0;    // rsrec_kubo_single_shot: orders added to the accumulators per pass (1..16; 0: SHOT_ORDERS_DEFAULT = 16; the same bits for every value)
    long opt_evolve_orders = 0;  // rsrec_chebyshev_evolve: 1 the accumulations ride in the per-order pass (fused), 2..16 a ring collects that many orders per accumulation pass (batched); 0: EVO_ORDERS_DEFAULT; the same bits for every value
    long opt_sitemap_orders = 0, opt_sitemap_vtile = 0;   // rsrec_chebyshev_site_map: orders PT added per pass (1..16) and vectors VT folded per pass (1..8), VT PT <= 16; 0: SITE_*_DEFAULT
    long opt_kubo_setgroup = 0;  // rsrec_kubo_moments_diag_tensor: sets of a vector contracted against one staged left tile (k_kubo_gram_diag_sets): 0 default (2), 1 every set by itself (k_kubo_gram_diag), 2 / 3 groups of at most that width
    int n_kubo_left_chunks = 0, kubo_lchunk_planned = 0;   // of the last Kubo moment call: left chunks formed over all its batches; left vectors per chunk as kubo_plan decided
    int kubo_diag_nvec = 0, kubo_diag_ll = 0;   // rsrec_kubo_moments_diag / _multi / _tensor: the call whose diagonal moments lie in d_kubo[4] (0: nothing resident; _multi: nvec * nout; _tensor: nvec * nout * nin)
    long opt_orth3 = 1;          // k_mfma_orth3: 1 one 512-register wave per SIMD (tables in registers), 2 two waves per SIMD (tables in LDS)
    long opt_graph = 1;          // level loop of small batches as one HIP graph: 0 never, 1 calls of up to 8 chains, 2 every single-batch call
    // A_n Gram folded into k_spmm5's epilogue (kernels_spmm5.hpp, S5Gram): a chain folds at a level when its region there has at least this
    // many groups of 8 atoms (0: always).  Measured per level on 16^3, 22^3 and 46^3: up to 84 groups the folded level is
    // 0.01-0.04 ms slower, at 139 and 212 groups the two are within the trace's 0.01 ms, from 308 groups on the folded level is faster in every
    // measurement -- 256 lies between.  Only operators that passed the Hermiticity check of rsrec_set_hamiltonian fold at all.
    long opt_s5_gram_min = 256;
    int ham_hermitian = 0;       // the operator as last set: one class, no hoh, and H_ji = H_ij^H block by block (see check_hermitian)
    std::vector<int> opp_slot;   // per slot: the slot that leads back (nbr(nbr(i, s), opp_slot[s]) == i for every atom i), empty: no unique map
    int opp_epoch = -1;          // lattice_epoch opp_slot was derived for
    DevBuf d_gram;               // the folded Gram's partials: [chain][group][spin][S5_GRAM_DOUBLES]
    double n_gram_folded = 0, n_gram_all = 0, n_gram_levels = 0;   // H|psi> launches of the last call in which some / every chain folded; all its launches
    // The captured level loop of the last small-batch block-Lanczos call (every SCF iteration repeats it with the same lattice, seeds,
    // depth and buffers; the operator's VALUES are read through device pointers and may change).  key = everything the nodes hold by value.
    hipGraphExec_t graph_exec = nullptr;
    std::vector<uintptr_t> graph_key;
    bool capturing = false;      // between hipStreamBeginCapture and hipStreamEndCapture: no timing events, no allocation
    // timing of last call
    double t_total_ms = 0, t_hop_ms = 0, t_rest_ms = 0, t_host_ms = 0;
    double t_rot_ms = 0;      // local-axis recursion: ms in k_rotate_coef (part of t_rest_ms)
    double t_evo_ms[2] = {0, 0};      // rsrec_chebyshev_evolve: ms in the step passes, in the record stage (their sum: t_rest_ms)
    double t_site_ms[2] = {0, 0};     // rsrec_chebyshev_site_map: ms in the accumulation passes, in the output stage (their sum: t_rest_ms)
    double t_shot_ms[2] = {0, 0};     // rsrec_kubo_single_shot: ms in the accumulation passes, in the final stage (their sum: t_rest_ms)
    double t_map_ms[3] = {0, 0, 0};   // rsrec_chebyshev_bloch_map: ms in the accumulation passes, the phase tables, the final sums (their sum: t_rest_ms)
    double n_hop_launch = 0, n_atom_steps = 0, n_block_mult = 0, n_hop_mfma_flop = 0;   // mfma_flop: matrix flops EXECUTED by the timed k_spmm5 launches
    double n_req_flop = 0;    // flops of H|psi> the operator's block structure requires (spin-diagonal blocks: half a zgemm), see required_hop_flops
    int hop_fuses_a = 1;      // 1: the timed H|psi> kernel also forms pmn and the A_n partial (VALU path); 0: pure SpMM (MFMA path)
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    // regions are purely topological: they are reused while the lattice and the seeds stay the same (every SCF iteration
    // of the reference calls recur_b with the same lattice%nn and lattice%irec)
    struct RegionEntry : RegionStats {      // a plan (region_plan.hpp) whose lists are on the device
        RegionKey key;
        std::vector<int> seeds;
        int epoch = 0;
        uint64_t serial = 0;                // from next_region_serial: names the entry in the captured graph's key (an address can come back)
        DevBuf order, cum;
    };
    std::vector<std::unique_ptr<RegionEntry>> region_cache;
    uint64_t next_region_serial = 1;        // never repeats
    int lattice_epoch = 0;
    const RegionEntry* cur_entry = nullptr;   // what upload_regions made current: the lists, tables and statistics every launch of the call reads
    std::vector<unsigned> spatial_key;   // per atom: position along a space-filling curve (locality hint for the saturated order)
    // coefficients left on the device by the last recursion call: 0 = none, 1 = block Lanczos (d_coefA = a_b, d_coefB = b2_b, never its
    // root), 2 = Chebyshev (d_mu = mu_n of all chains)
    int res_kind = 0, res_n = 0, res_lld = 0;
    bool res_seeded = false;            // the resident chains come from a seeded (pair) call, not from one chain per site
    // library-level communicator (RCCL, bound with dlopen at rsrec_comm_init): the one exchange of the path without MPI or torch
    void* comm = nullptr;
    int comm_rank = 0, comm_nranks = 1;
    DevBuf d_comm;               // staging buffer of rsrec_allreduce_sum on host arrays
    ~rsrec_handle();
};

namespace {

// Every option of rsrec_set_option, once: the key is looked up here, and the captured level loop is keyed by all of them (see run_block_lanczos).
struct OptionEntry { const char* name; long rsrec_handle::*member; };
const OptionEntry OPTIONS[] = {
    {"batch", &rsrec_handle::opt_batch},
    {"kernels", &rsrec_handle::opt_kernels},
    {"nblk", &rsrec_handle::opt_nblk},
    {"spmm5", &rsrec_handle::opt_spmm5},
    {"chain_fold", &rsrec_handle::opt_chain_fold},
    {"s5_cap", &rsrec_handle::opt_s5_cap},
    {"s5_lds", &rsrec_handle::opt_s5_lds},
    {"s5_queue", &rsrec_handle::opt_s5_queue},
    {"cheb_fused", &rsrec_handle::opt_cheb_fused},
    {"side_stream", &rsrec_handle::opt_side},
    {"graph", &rsrec_handle::opt_graph},
    {"orth3", &rsrec_handle::opt_orth3},
    {"s5_waves", &rsrec_handle::opt_s5_waves},
    {"s5_split", &rsrec_handle::opt_s5_split},
    {"orth_oop", &rsrec_handle::opt_orth_oop},
    {"sat_pct", &rsrec_handle::opt_sat_pct},
    {"kubo_lchunk", &rsrec_handle::opt_kubo_lchunk},
    {"kubo_vbatch", &rsrec_handle::opt_kubo_vbatch},
    {"kubo_setgroup", &rsrec_handle::opt_kubo_setgroup},
    {"shot_orders", &rsrec_handle::opt_shot_orders},
    {"sitemap_orders", &rsrec_handle::opt_sitemap_orders},
    {"evolve_orders", &rsrec_handle::opt_evolve_orders},
    {"sitemap_vtile", &rsrec_handle::opt_sitemap_vtile},
    {"lattice_vbatch", &rsrec_handle::opt_lattice_vbatch},
    {"blochmap_orders", &rsrec_handle::opt_blochmap_orders},
    {"blochmap_kchunk", &rsrec_handle::opt_blochmap_kchunk},
    {"s5_host_emit", &rsrec_handle::opt_s5_host_emit},
    {"s5_octet", &rsrec_handle::opt_s5_octet},
    {"s5_spin_xcd", &rsrec_handle::opt_s5_spin_xcd},
    {"s5_run_min", &rsrec_handle::opt_s5_run_min},
    {"s5_gram_min", &rsrec_handle::opt_s5_gram_min},
};

int fail(rsrec_t* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return code;
}

#define HIPCK(h, call)                                                                                         \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess) return fail(h, RSREC_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

hipEvent_t next_event(rsrec_t* h) {
    static const bool off = getenv("RSREC_NO_EVENTS") != nullptr;      // diagnostics only
    if (off || h->capturing) return nullptr;
    if (h->ev_used == h->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        h->ev_pool.push_back(e);
    }
    hipEvent_t e = h->ev_pool[h->ev_used++];
    (void)hipEventRecord(e, h->stream);
    return e;
}

// Host <-> device transfers of per-call data go through one pinned staging buffer.  hipMemcpyAsync straight from/to the
// caller's pageable arrays (freshly allocated numpy / Fortran ALLOCATE memory) was measured at 60-90 ms PER CALL for a 259 KB
// coefficient download on the MI355X boxes (rocprofv3 --hip-trace: the time is inside hipMemcpyAsync, the GPU idles) --
// four times the whole single-site recursion.  Staged copies are synchronous by construction (stream order + one wait).
constexpr size_t PIN_BYTES = (size_t)8 << 20;
int pin_ready(rsrec_t* h) {
    if (h->pin) return RSREC_OK;
    if (hipHostMalloc(&h->pin, PIN_BYTES, hipHostMallocDefault) != hipSuccess) { h->pin = nullptr; return fail(h, RSREC_ERR_DEVICE, "hipHostMalloc of the staging buffer failed"); }
    h->pin_bytes = PIN_BYTES;
    return RSREC_OK;
}
// device -> caller memory; waits for everything queued on the stream before it
constexpr size_t PIN_MAX_XFER = (size_t)8 << 20;     // larger transfers are bandwidth-, not latency-bound: direct copy (no extra host memcpy)
int xfer_d2h(rsrec_t* h, void* dst, const void* src_dev, size_t bytes) {
    if (bytes > PIN_MAX_XFER) {
        HIPCK(h, hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        return RSREC_OK;
    }
    int rc = pin_ready(h);
    if (rc) return rc;
    for (size_t off = 0; off < bytes; off += h->pin_bytes) {
        const size_t n = std::min(h->pin_bytes, bytes - off);
        HIPCK(h, hipMemcpyAsync(h->pin, static_cast<const char*>(src_dev) + off, n, hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        memcpy(static_cast<char*>(dst) + off, h->pin, n);
    }
    return RSREC_OK;
}
// caller memory -> device; returns when the data is on the device (the staging buffer is free again)
int xfer_h2d(rsrec_t* h, void* dst_dev, const void* src, size_t bytes) {
    if (bytes > PIN_MAX_XFER) {
        HIPCK(h, hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        return RSREC_OK;
    }
    int rc = pin_ready(h);
    if (rc) return rc;
    for (size_t off = 0; off < bytes; off += h->pin_bytes) {
        const size_t n = std::min(h->pin_bytes, bytes - off);
        memcpy(h->pin, static_cast<const char*>(src) + off, n);
        HIPCK(h, hipMemcpyAsync(static_cast<char*>(dst_dev) + off, h->pin, n, hipMemcpyHostToDevice, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
    }
    return RSREC_OK;
}
#define XFER(call) do { int rc__ = (call); if (rc__) return rc__; } while (0)

LatticeView lattice_view(const rsrec_t* h) {
    return LatticeView{h->kk, h->nslots, h->nmax, h->ntype, h->nbr.data(), h->iz0.data(), h->radj_ptr.data(), h->radj.data(), h->spatial_key.data()};
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
extern "C" int rsrec_version(void) { return 101; }

extern "C" int rsrec_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// RSREC_REPORT set in the environment: one line of the handle's counters when the process exits -- the evidence a host that cannot
// ask (the reference's unmodified main program behind the shadow modules, fortran/build_dropin.sh) leaves in its log that its
// operator was assembled on the device and taken from there, and that the LDOS stage ran there.  Host-side counters only: no HIP call
// is made from the exit handler.
static rsrec_handle* g_report_handle = nullptr;
static void report_at_exit() {
    const rsrec_handle* h = g_report_handle;
    if (!h) return;
    std::printf("rsrec report: library_calls=%ld device_assemblies=%ld operator_arrays_from_device=%d device_ldos_calls=%ld\n", h->n_recursion_calls, h->n_asm_calls,
                h->n_asm_reused, h->n_ldos_calls);
    std::fflush(stdout);
}

extern "C" int rsrec_create(rsrec_t** out, int device) {
    if (!out) return RSREC_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RSREC_ERR_DEVICE;   // no CPU fallback by design
    if (device < 0 || device >= ndev) return RSREC_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return RSREC_ERR_DEVICE;
    rsrec_t* h = new rsrec_handle();
    h->device = device;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return RSREC_ERR_DEVICE; }
    if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->n_cu <= 0) h->n_cu = 256;
    *out = h;
    if (getenv("RSREC_REPORT") && !g_report_handle) {
        static bool registered = false;
        if (!registered) { registered = std::atexit(report_at_exit) == 0; }
        g_report_handle = h;
    }
    return RSREC_OK;
}

// Every hipFree of the handle happens in here or in the members' destructors right behind it, with the handle's device current.  Also
// safe on a handle that never got its stream (rsrec_create's early delete): nothing below touches the device then.
rsrec_handle::~rsrec_handle() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    (void)rsrec_comm_destroy(this);
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    for (hipStream_t s : {stream, copy_stream, side_stream, oct_stream}) if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : {ev_green[0], ev_green[1], ev_orth, ev_bred, ev_oct_in, ev_oct_out}) if (e) (void)hipEventDestroy(e);
    if (pin) (void)hipHostFree(pin);
}

extern "C" int rsrec_destroy(rsrec_t* h) {
    if (!h) return RSREC_ERR_ARG;
    if (g_report_handle == h) { report_at_exit(); g_report_handle = nullptr; }
    delete h;
    return RSREC_OK;
}

extern "C" int rsrec_last_error(rsrec_t* h, char* buf, size_t n) {
    if (!h || !buf || n == 0) return RSREC_ERR_ARG;
    snprintf(buf, n, "%s", h->err.c_str());
    return RSREC_OK;
}

extern "C" int rsrec_set_option(rsrec_t* h, const char* key, long value) {
    if (!h || !key) return RSREC_ERR_ARG;
    for (const OptionEntry& o : OPTIONS)
        if (!strcmp(key, o.name)) { h->*o.member = value; return RSREC_OK; }
    return fail(h, RSREC_ERR_ARG, "unknown option '%s'", key);
}

extern "C" int rsrec_get_timing(rsrec_t* h, double* out, int n) {
    if (!h || !out) return RSREC_ERR_ARG;
    const double v[25] = {h->t_total_ms, h->t_hop_ms, h->n_hop_launch, h->n_atom_steps, h->n_block_mult, h->t_rest_ms, h->t_host_ms, (double)h->hop_fuses_a, h->n_hop_mfma_flop,
                          h->n_req_flop, (double)h->n_asm_reused, (double)h->n_octet_launch, h->t_rot_ms, h->n_gram_folded, h->t_map_ms[0], h->t_map_ms[1], h->t_map_ms[2], h->t_shot_ms[0], h->t_shot_ms[1], (double)h->n_kubo_left_chunks, (double)h->kubo_lchunk_planned, h->t_site_ms[0], h->t_site_ms[1], h->t_evo_ms[0], h->t_evo_ms[1]};
    for (int i = 0; i < n && i < 25; ++i) out[i] = v[i];
    return RSREC_OK;
}

extern "C" void rsrec_site_partition(int rank, int nprocs, int nsites, int* start_atom, int* end_atom) {
    // get_mpi_variables, mpi.f90:37-46
    int per = nsites / nprocs;
    const int rem = nsites % nprocs;
    int start;
    if (rank < rem) { per += 1; start = rank * per + 1; }
    else start = rank * per + rem + 1;
    *start_atom = start;
    *end_atom = start + per - 1;
}

static void release_graph(rsrec_t* h) {
    if (h->graph_exec) { (void)hipDeviceSynchronize(); (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
    h->graph_key.clear();
}

// cached regions (device order lists) of lattice epochs that ended; the stream is idle between calls.  The captured level loop holds
// the region lists, the lattice tables and their dimensions BY VALUE: it goes with them (a new RegionEntry / hipMalloc of the same
// size commonly returns the old address, so pointers alone cannot tell a new lattice from the old one)
static void release_regions(rsrec_t* h) {
    release_graph(h);
    if (!h->region_cache.empty()) (void)hipDeviceSynchronize();
    h->region_cache.clear();
    h->cur_entry = nullptr;
}

extern "C" int rsrec_set_lattice(rsrec_t* h, int kk, int nncols, const int32_t* nn, const int32_t* iz, int nmax, int ntype) {
    if (!h || !nn || !iz || kk <= 0 || nncols < 1 || nmax < 0 || nmax > kk || ntype < 1) return fail(h, RSREC_ERR_ARG, "rsrec_set_lattice: bad argument");
    HIPCK(h, hipSetDevice(h->device));
    // unchanged lattice (every SCF iteration of the reference calls the drivers with the same lattice%nn): keep the device tables
    // and, above all, the cached regions -- building them costs as much host time as the recursion costs device time
    if (h->have_lattice && kk == h->kk && nncols == h->lat_nncols && nmax == h->nmax && ntype == h->ntype &&
        h->lat_nn.size() == (size_t)kk * nncols && std::memcmp(h->lat_nn.data(), nn, h->lat_nn.size() * sizeof(int32_t)) == 0 &&
        std::memcmp(h->lat_iz.data(), iz, (size_t)kk * sizeof(int32_t)) == 0)
        return RSREC_OK;
    // validate and convert into local tables first: a refused call leaves the handle as it was
    int nslots = 1;
    for (int i = 0; i < kk; ++i) {
        const int nr = nn[i];
        if (nr < 0 || nr > nncols) return fail(h, RSREC_ERR_ARG, "rsrec_set_lattice: nn(%d,1)=%d outside 0..%d", i + 1, nr, nncols);
        nslots = std::max(nslots, nr);
        if (iz[i] < 1 || iz[i] > ntype) return fail(h, RSREC_ERR_ARG, "rsrec_set_lattice: iz(%d)=%d outside 1..%d", i + 1, iz[i], ntype);
    }
    std::vector<int> nbr_new((size_t)kk * nslots, -1), iz_new(kk);
    for (int i = 0; i < kk; ++i) {
        iz_new[i] = iz[i] - 1;
        nbr_new[(size_t)i * nslots] = i;
        const int nr = nn[i];
        for (int j = 1; j < nr; ++j) {   // slots 2..nn(i,1) of the reference (recursion.f90:1614)
            const int n = nn[(size_t)i + (size_t)kk * j];
            if (n == 0) continue;
            if (n < 0 || n > kk) return fail(h, RSREC_ERR_ARG, "rsrec_set_lattice: nn(%d,%d)=%d outside 0..%d", i + 1, j + 1, n, kk);
            nbr_new[(size_t)i * nslots + j] = n - 1;
        }
    }
    // from here on the handle changes: until the last table is uploaded it holds no lattice (a failed upload must not leave the
    // unchanged-lattice shortcut above pointing at half-replaced tables), and the cached regions of the old lattice are released
    h->have_lattice = false;
    h->have_ham = false;
    h->kubo_diag_nvec = h->kubo_diag_ll = 0;                     // (resident Kubo moments belong to the lattice they were computed on)
    h->lat_nn.clear(); h->lat_iz.clear();
    release_regions(h);
    h->kk = kk; h->nslots = nslots; h->nmax = nmax; h->ntype = ntype;
    h->nbr.swap(nbr_new);
    h->iz0.swap(iz_new);
    reverse_adjacency(kk, nslots, h->nbr.data(), h->radj_ptr, h->radj);
    HIPCK(h, h->d_nbr.reserve(h->nbr.size() * sizeof(int)));
    HIPCK(h, h->d_iz.reserve((size_t)kk * sizeof(int)));
    HIPCK(h, hipMemcpy(h->d_nbr.p, h->nbr.data(), h->nbr.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCK(h, hipMemcpy(h->d_iz.p, h->iz0.data(), (size_t)kk * sizeof(int), hipMemcpyHostToDevice));
    {
        // (kk+1) x (nslots+2): absent neighbours and the extra row -> zero block; column nslots = the atom itself (extra on-site slot),
        // column nslots + 1 = zero block (null entries of the k_spmm5 schedule)
        std::vector<int> n5((size_t)(kk + 1) * (nslots + 2), kk);
        for (int i = 0; i < kk; ++i) {
            for (int j = 0; j < nslots; ++j) { const int n = h->nbr[(size_t)i * nslots + j]; if (n >= 0) n5[(size_t)i * (nslots + 2) + j] = n; }
            n5[(size_t)i * (nslots + 2) + nslots] = i;
        }
        HIPCK(h, h->d_nbr5.reserve(n5.size() * sizeof(int)));
        HIPCK(h, hipMemcpy(h->d_nbr5.p, n5.data(), n5.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    spatial_key_from_graph(lattice_view(h), h->spatial_key);
    h->lat_nn.assign(nn, nn + (size_t)kk * nncols);
    h->lat_iz.assign(iz, iz + kk);
    h->lat_nncols = nncols;
    h->lat_cr.clear();
    h->have_lattice = true;
    h->lattice_epoch++;
    h->have_ham = false;   // operator tables depend on nmax/ntype: must be set again
    return RSREC_OK;
}

extern "C" int rsrec_set_positions(rsrec_t* h, const double* cr) {
    if (!h || !cr) return fail(h, RSREC_ERR_ARG, "rsrec_set_positions: bad argument");
    if (!h->have_lattice) return fail(h, RSREC_ERR_ARG, "rsrec_set_positions: call rsrec_set_lattice first");
    const int kk = h->kk;
    if (h->lat_cr.size() == 3 * (size_t)kk && std::memcmp(h->lat_cr.data(), cr, h->lat_cr.size() * sizeof(double)) == 0) return RSREC_OK;
    h->lat_cr.assign(cr, cr + 3 * (size_t)kk);
    spatial_key_from_positions(kk, cr, h->spatial_key);
    h->lattice_epoch++;        // cached region orders were built with the old keys: they can never match again
    release_regions(h);
    return RSREC_OK;
}

namespace {

// Is the operator as set Hermitian, H_ji = H_ij^H?  Asked of operators with one class and no hoh only (what the Gram fold serves).  The
// slot that leads back comes from the neighbour table: slot s of atom i leads to j, and s' is the slot of j that holds i -- the same s'
// for every atom, and the only one, or there is no map and the answer is no.  Then ee[s'] = ee[s]^H and ee[0] + lsham Hermitian (st: the
// stencil with l.s folded into slot 0), to 1e-12 of the largest element.
bool check_hermitian(rsrec_t* h, const double* st) {
    if (h->ntype != 1 || h->nmax != 0 || h->hoh) return false;
    const int ns = h->nslots, kk = h->kk;
    if (h->opp_epoch != h->lattice_epoch) {
        h->opp_epoch = h->lattice_epoch;
        std::vector<int> opp(ns, -1);
        bool ok = true;
        opp[0] = 0;
        for (int i = 0; i < kk && ok; ++i)
            for (int s = 1; s < ns && ok; ++s) {
                const int j = h->nbr[(size_t)i * ns + s];
                if (j < 0) continue;
                int back = -1, nback = 0;
                for (int q = 0; q < ns; ++q) if (h->nbr[(size_t)j * ns + q] == i) { back = q; ++nback; }
                if (nback != 1 || back == 0 || (opp[s] >= 0 && opp[s] != back)) ok = false;
                else opp[s] = back;
            }
        for (int s = 0; s < ns && ok; ++s) if (opp[s] < 0 || opp[opp[s]] != s) ok = false;
        if (!ok) opp.clear();
        h->opp_slot.swap(opp);
    }
    if (h->opp_slot.empty()) return false;
    const size_t B = 2 * (size_t)BLK;
    double big = 0.0;
    for (size_t e = 0; e < B * ns; ++e) big = std::max(big, std::fabs(st[e]));
    const double tol = 1e-12 * big;
    for (int s = 0; s < ns; ++s) {
        const double *a = st + B * s, *b = st + B * h->opp_slot[s];
        for (int r = 0; r < NB; ++r)
            for (int c = 0; c < NB; ++c) {
                const double dr = b[2 * (c + NB * r)] - a[2 * (r + NB * c)], di = b[2 * (c + NB * r) + 1] + a[2 * (r + NB * c) + 1];
                if (!(std::fabs(dr) <= tol && std::fabs(di) <= tol)) return false;
            }
    }
    return true;
}

}  // namespace

extern "C" int rsrec_set_hamiltonian(rsrec_t* h, int nslots, int hoh, int nsp, const double* ee, const double* lsham, const double* eeo,
                                     const double* enim, const double* hall, const double* hallo) {
    if (!h) return RSREC_ERR_ARG;
    if (!h->have_lattice) return fail(h, RSREC_ERR_ARG, "rsrec_set_hamiltonian: call rsrec_set_lattice first");
    if (!ee || !lsham || nslots < h->nslots) return fail(h, RSREC_ERR_ARG, "rsrec_set_hamiltonian: ee/lsham missing or nslots=%d < lattice slots %d", nslots, h->nslots);
    if (hoh && (!eeo || !enim)) return fail(h, RSREC_ERR_ARG, "rsrec_set_hamiltonian: hoh requires eeo and enim");
    if (h->nmax > 0 && (!hall || (hoh && !hallo))) return fail(h, RSREC_ERR_ARG, "rsrec_set_hamiltonian: nmax>0 requires hall (and hallo with hoh)");
    HIPCK(h, hipSetDevice(h->device));
    const size_t B = 2 * (size_t)BLK;   // doubles per block
    const int ntype = h->ntype, nmax = h->nmax;
    h->hslots = nslots; h->hoh = hoh ? 1 : 0; h->nsp = nsp;
    h->kubo_diag_nvec = h->kubo_diag_ll = 0;                     // (resident Kubo moments belong to the Hamiltonian they were computed with)
    h->host_ee.assign(ee, ee + 2 * (size_t)BLK * nslots * h->ntype);
    h->host_lsham.assign(lsham, lsham + 2 * (size_t)BLK * h->ntype);
    h->host_eeo.clear(); h->host_enim.clear(); h->host_hall.clear(); h->host_hallo.clear();
    if (hoh) { h->host_eeo.assign(eeo, eeo + 2 * (size_t)BLK * nslots * h->ntype); h->host_enim.assign(enim, enim + 2 * (size_t)BLK * h->ntype); }
    if (h->nmax > 0) { h->host_hall.assign(hall, hall + 2 * (size_t)BLK * nslots * h->nmax); if (hoh) h->host_hallo.assign(hallo, hallo + 2 * (size_t)BLK * nslots * h->nmax); }
    h->s5_la_ok = 0;
    // stencil with the on-site spin-orbit block folded into slot 0 (locham = ee(:,:,1,ih) + lsham(:,:,ih), recursion.f90:1608)
    std::vector<double> st(ee, ee + B * nslots * ntype);
    if (!hoh)
        for (int t = 0; t < ntype; ++t)
            for (size_t e = 0; e < B; ++e) st[B * nslots * t + e] += lsham[B * t + e];
    h->ham_hermitian = check_hermitian(h, st.data()) ? 1 : 0;
    // Arrays that rsrec_assemble_blocks produced (the caller hands back, bit for bit, what it was given) are already on the device:
    // a device-to-device copy (+ the l.s fold) replaces the upload.  Anything else -- arrays built on the host, or edited since -- is uploaded.
    h->n_asm_reused = 0;
    auto resident = [&](int part, int which, const double* arr, int ncls) -> const double* {
        const size_t n = B * nslots * ncls;
        if (!arr || h->asm_nslots[part] != nslots || h->asm_ncls[part] != ncls || h->asm_host[part][which].size() != n) return nullptr;
        if (std::memcmp(arr, h->asm_host[part][which].data(), n * 8) != 0) return nullptr;
        h->n_asm_reused++;
        return h->d_asm[part][which].as<double>();
    };
    auto place = [&](DevBuf& dst, const double* dev_src, const double* host_src, size_t n) -> hipError_t {
        hipError_t e = dst.reserve(n * 8);
        if (e != hipSuccess) return e;
        if (dev_src) return hipMemcpyAsync(dst.p, dev_src, n * 8, hipMemcpyDeviceToDevice, h->stream);
        return hipMemcpy(dst.p, host_src, n * 8, hipMemcpyHostToDevice);
    };
    HIPCK(h, h->d_lsham.reserve(B * ntype * 8));
    HIPCK(h, hipMemcpy(h->d_lsham.p, lsham, B * ntype * 8, hipMemcpyHostToDevice));
    {
        const double* dev = resident(0, 0, ee, ntype);
        HIPCK(h, place(h->d_hst, dev, st.data(), st.size()));
        if (dev && !hoh) k_fold_onsite<<<ntype, 324, 0, h->stream>>>(h->d_hst.as<double2>(), nslots, h->d_lsham.as<double2>(), nullptr);
    }
    std::vector<double> loc;
    if (nmax > 0) {
        loc.assign(hall, hall + B * nslots * nmax);
        if (!hoh)
            for (int i = 0; i < nmax; ++i)
                for (size_t e = 0; e < B; ++e) loc[B * nslots * i + e] += lsham[B * h->iz0[i] + e];   // :1582
        const double* dev = resident(1, 0, hall, nmax);
        HIPCK(h, place(h->d_hloc, dev, loc.data(), loc.size()));
        if (dev && !hoh) k_fold_onsite<<<nmax, 324, 0, h->stream>>>(h->d_hloc.as<double2>(), nslots, h->d_lsham.as<double2>(), h->d_iz.as<int>());
    }
    if (hoh) {
        HIPCK(h, place(h->d_host, resident(0, 1, eeo, ntype), eeo, B * nslots * ntype));
        HIPCK(h, h->d_enim.reserve(B * ntype * 8));
        HIPCK(h, hipMemcpy(h->d_enim.p, enim, B * ntype * 8, hipMemcpyHostToDevice));
        if (nmax > 0) HIPCK(h, place(h->d_holoc, resident(1, 1, hallo, nmax), hallo, B * nslots * nmax));
    }
    HIPCK(h, hipGetLastError());
    // MFMA-fragment form of the same operator tables.  k_spmm5's streams are assembled on the DEVICE from the raw blocks uploaded above
    // (Spmm5Operator::build -> k_s5_emit; option s5_host_emit = 1: on the host, the round-2 path, kept as the cross-check).  k_spmm4's
    // tables (small launches of the plain operator only) are built when a call first needs them (ensure_s4).
    {
        h->s4_built_split = 0; h->s5_built = 0;
        if (h->nslots + 1 <= S4_MAXSLOTS) {
            h->host_st.swap(st);
            h->host_loc.swap(loc);
            const double* dev[6] = {h->d_hst.as<double>(), h->d_hloc.as<double>(), h->d_host.as<double>(), h->d_holoc.as<double>(), h->d_enim.as<double>(), h->d_lsham.as<double>()};
            const char* msg = h->s5_op.build(h->nslots, nslots, ntype, nmax, h->hoh, h->host_st.data(), nmax > 0 ? h->host_loc.data() : nullptr, hoh ? eeo : nullptr,
                                             (hoh && nmax > 0) ? hallo : nullptr, hoh ? enim : nullptr, lsham, h->iz0.data(), h->opt_s5_host_emit ? nullptr : dev, h->stream);
            if (msg) return fail(h, RSREC_ERR_DEVICE, "rsrec_set_hamiltonian: %s", msg);
            h->s5_built = 1;
        }
    }
    h->have_ham = true;
    return RSREC_OK;
}

extern "C" int rsrec_assemble_blocks(rsrec_t* h, int part, int ncls, int nslots, int hoh, const double* hmag, const int32_t* nbr_type, const double* obarm, int ntype,
                                     double* blocks, double* blocks_o) {
    if (!h) return RSREC_ERR_ARG;
    if (part < 0 || part > 1 || ncls < 1 || nslots < 1 || !hmag || !blocks) return fail(h, RSREC_ERR_ARG, "rsrec_assemble_blocks: part=%d ncls=%d nslots=%d or a missing array", part, ncls, nslots);
    if (hoh && (!nbr_type || !obarm || !blocks_o || ntype < 1)) return fail(h, RSREC_ERR_ARG, "rsrec_assemble_blocks: hoh needs nbr_type, obarm (ntype=%d) and blocks_o", ntype);
    if (hoh)
        for (size_t q = 0; q < (size_t)ncls * nslots; ++q)
            if (nbr_type[q] < 0 || nbr_type[q] > ntype) return fail(h, RSREC_ERR_ARG, "rsrec_assemble_blocks: nbr_type[%zu]=%d outside 0..%d", q, nbr_type[q], ntype);
    HIPCK(h, hipSetDevice(h->device));
    h->n_asm_calls++;
    h->asm_nslots[part] = h->asm_ncls[part] = 0;          // nothing valid while this runs
    const size_t nblk = (size_t)ncls * nslots, hm_bytes = nblk * 4 * 81 * 16, ty_bytes = nblk * 4, ob_bytes = hoh ? (size_t)ntype * 324 * 16 : 0;
    const size_t ty_off = (hm_bytes + 255) / 256 * 256, ob_off = ty_off + (ty_bytes + 255) / 256 * 256;
    HIPCK(h, h->d_asm_in.reserve(ob_off + ob_bytes + 256));
    char* in = h->d_asm_in.as<char>();
    XFER(xfer_h2d(h, in, hmag, hm_bytes));
    if (hoh) { XFER(xfer_h2d(h, in + ty_off, nbr_type, ty_bytes)); XFER(xfer_h2d(h, in + ob_off, obarm, ob_bytes)); }
    HIPCK(h, h->d_asm[part][0].reserve(nblk * 324 * 16));
    if (hoh) HIPCK(h, h->d_asm[part][1].reserve(nblk * 324 * 16));
    k_assemble_blocks<<<dim3(nslots, ncls), 384, 0, h->stream>>>(reinterpret_cast<const double2*>(in), reinterpret_cast<const int*>(in + ty_off),
                                                                 reinterpret_cast<const double2*>(in + ob_off), nslots, hoh ? 1 : 0, h->d_asm[part][0].as<double2>(),
                                                                 hoh ? h->d_asm[part][1].as<double2>() : nullptr);
    HIPCK(h, hipGetLastError());
    XFER(xfer_d2h(h, blocks, h->d_asm[part][0].p, nblk * 324 * 16));
    if (hoh) XFER(xfer_d2h(h, blocks_o, h->d_asm[part][1].p, nblk * 324 * 16));
    h->asm_host[part][0].assign(blocks, blocks + nblk * 648);
    if (hoh) h->asm_host[part][1].assign(blocks_o, blocks_o + nblk * 648); else h->asm_host[part][1].clear();
    h->asm_nslots[part] = nslots; h->asm_ncls[part] = ncls; h->asm_hoh[part] = hoh ? 1 : 0;
    return RSREC_OK;
}

namespace {

DevProblem make_problem(const rsrec_t* h) {
    DevProblem P;
    P.kk = h->kk; P.nslots = h->nslots; P.hstride = h->hslots; P.nmax = h->nmax; P.hoh = h->hoh;
    P.nbr = h->d_nbr.as<int>(); P.iz = h->d_iz.as<int>();
    P.h_st = h->d_hst.as<double2>(); P.h_loc = h->d_hloc.as<double2>();
    P.ho_st = h->d_host.as<double2>(); P.ho_loc = h->d_holoc.as<double2>();
    P.enim = h->d_enim.as<double2>(); P.lsham = h->d_lsham.as<double2>();
    return P;
}

// Buffers a Kubo call keeps for the next one: d_kubo (rsrec_kubo_moments: work vectors and moment matrices, tens of GB) and d_cond
// (rsrec_kubo_integrand: tables, S / D planes, partials; up to ~10 GB at RSREC_COND_LL_MAX).  Every entry point that reserves large
// buffers of its own gives them back before it does, so that it plans on memory that is really free.
void release_kubo_buffers(rsrec_t* h, bool moments, bool integrand) {
    if (moments) { for (auto& kb : h->d_kubo) kb.release(); h->kubo_diag_nvec = h->kubo_diag_ll = 0; }
    if (integrand) { for (auto& cb : h->d_cond) cb.release(); for (auto& cb : h->d_ctens) cb.release(); for (auto& cb : h->d_opt) cb.release(); }
}

struct BatchPlan {
    int batch = 1, nblk = 1;
};

// how many chains are advanced together, and how many workgroups each gets
int plan_batch(rsrec_t* h, int nchains, int nvec, size_t vec_elems_per_chain, BatchPlan& bp, size_t extra_bytes_per_chain = 0) {
    release_kubo_buffers(h, true, true);                         // (a Kubo call keeps its buffers for the next one; the recursion takes the memory back)
    size_t free_b = 0, total_b = 0;
    HIPCK(h, hipMemGetInfo(&free_b, &total_b));
    size_t reusable = 0;
    for (int v = 0; v < 5; ++v) reusable += h->d_vec[v].bytes;
    if (extra_bytes_per_chain) reusable += h->d_gram.bytes;        // (a call that does not fold leaves the buffer alone: it is not free memory)
    const double per_chain = (double)nvec * vec_elems_per_chain * sizeof(double2) + (double)h->kk * 4 + 4096 + (double)extra_bytes_per_chain;
    long cap = (long)((0.85 * (double)(free_b + reusable)) / per_chain);
    if (cap < 1) return fail(h, RSREC_ERR_DEVICE, "not enough device memory for one chain (%.1f MB needed, %.1f MB free)", per_chain / 1e6, free_b / 1e6);
    long b = h->opt_batch > 0 ? h->opt_batch : 64;
    b = std::min<long>(b, cap);
    b = std::min<long>(b, nchains);
    bp.batch = (int)std::max<long>(b, 1);
    long nblk = h->opt_nblk > 0 ? h->opt_nblk : std::max<long>(2048 / bp.batch, 16);
    nblk = std::min<long>(nblk, 256);
    nblk = std::min<long>(nblk, (h->kk + TILE_ATOMS - 1) / TILE_ATOMS);
    bp.nblk = (int)std::max<long>(nblk, 1);
    return RSREC_OK;
}

// The regions of one batch on the device, current for the launches that follow (h->cur_entry).  seeds0: [nb][nseed] 0-based.  Regions are purely
// topological: an entry is reused while the lattice and the seeds stay the same (every SCF iteration of the reference calls recur_b with the same
// lattice%nn and lattice%irec).  A new entry joins the cache once its lists are on the device: a failure leaves cache and current entry as they were.
constexpr size_t REGION_CACHE_MAX = 256;
int upload_regions(rsrec_t* h, const int* seeds0, int nb, int nseed, int nlev, int napply, bool two_pass, bool grouped) {
    const RegionKey key{nb, nseed, nlev, napply, two_pass, grouped, (int)std::min<long>(100, std::max<long>(1, h->opt_sat_pct))};
    for (const auto& e : h->region_cache)
        if (e->epoch == h->lattice_epoch && e->key == key && std::equal(e->seeds.begin(), e->seeds.end(), seeds0)) { h->cur_entry = e.get(); return RSREC_OK; }
    RegionPlan plan;
    const std::string refused = plan_regions(lattice_view(h), key, seeds0, plan);
    if (!refused.empty()) return fail(h, RSREC_ERR_ARG, "%s", refused.c_str());
    auto e = std::make_unique<rsrec_handle::RegionEntry>();
    static_cast<RegionStats&>(*e) = std::move(static_cast<RegionStats&>(plan));
    e->key = key; e->epoch = h->lattice_epoch; e->serial = h->next_region_serial++; e->seeds.assign(seeds0, seeds0 + (size_t)nb * nseed);
    HIPCK(h, e->order.reserve(plan.order.size() * 4));
    HIPCK(h, e->cum.reserve(plan.cum.size() * 4));
    XFER(xfer_h2d(h, e->order.p, plan.order.data(), plan.order.size() * 4));
    XFER(xfer_h2d(h, e->cum.p, plan.cum.data(), plan.cum.size() * 4));
    HIPCK(h, hipStreamSynchronize(h->stream));   // the plan's order / cum are local
    if (h->region_cache.size() >= REGION_CACHE_MAX) release_regions(h);   // bounded: drop everything, the captured level loop with the lists it points into
    h->region_cache.push_back(std::move(e));
    h->cur_entry = h->region_cache.back().get();
    return RSREC_OK;
}

// Flops of the H|psi> applications of the current region entry that the operator's block structure requires: the reference multiplies
// full 18x18 blocks (zgemm, recursion.f90:1618: 46 656 flop each), but the hopping blocks of a collinear magnet are spin-diagonal
// (hamiltonian.f90:1553-1617) and need half of that.  This -- not the reference's count -- is what a roofline fraction is measured in.
double required_hop_flops(const rsrec_t* h, const Spmm5Operator& op) {
    if (!h->cur_entry) return 0.0;
    const int ntau = h->nmax + h->ntype, nfs = h->nslots + 1;
    const std::vector<double>& H = h->cur_entry->mult_hist;
    if (H.size() != (size_t)2 * ntau * nfs) return 0.0;
    double f = 0.0;
    for (int pass = 0; pass < 2; ++pass)
        for (int t = 0; t < ntau; ++t)
            for (int s = 0; s < nfs; ++s) {
                const double n = H[((size_t)pass * ntau + t) * nfs + s];
                if (n == 0.0) continue;
                const double w = (op.mixing.empty() || op.ntau != ntau || op.nslots != h->nslots) ? 46656.0 : op.required_flops(pass, t, s);
                f += n * (w > 0.0 ? w : 46656.0);
            }
    return f;
}

void reset_timing(rsrec_t* h) {
    h->t_total_ms = h->t_hop_ms = h->t_rest_ms = h->t_host_ms = h->t_rot_ms = 0;
    h->t_map_ms[0] = h->t_map_ms[1] = h->t_map_ms[2] = 0;
    h->t_shot_ms[0] = h->t_shot_ms[1] = 0;
    h->t_site_ms[0] = h->t_site_ms[1] = 0;
    h->t_evo_ms[0] = h->t_evo_ms[1] = 0;
    h->n_kubo_left_chunks = h->kubo_lchunk_planned = 0;
    h->n_hop_launch = h->n_atom_steps = h->n_block_mult = h->n_hop_mfma_flop = h->n_req_flop = 0;
    h->n_octet_launch = 0;
    h->n_gram_folded = h->n_gram_all = h->n_gram_levels = 0;
    h->ev_used = 0;
    h->n_recursion_calls++;          // (every timed entry point: recursions, Green / LDOS stages, Kubo moments)
}

double ev_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (!a || !b || hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.0;
    return ms;
}

int check_ready(rsrec_t* h, const char* who) {
    if (!h) return RSREC_ERR_ARG;
    if (!h->have_lattice || !h->have_ham) return fail(h, RSREC_ERR_ARG, "%s: lattice and hamiltonian must be set first", who);
    return RSREC_OK;
}

// seed atoms of a call as the caller numbers them: lo..kk (1-based; rsrec_kubo_moments also takes 0 = unused entry)
int check_seeds(rsrec_t* h, const char* who, const int32_t* atoms, size_t n, int lo) {
    for (size_t q = 0; q < n; ++q)
        if (atoms[q] < lo || atoms[q] > h->kk) return fail(h, RSREC_ERR_ARG, "%s: seed atom %d outside %d..%d", who, atoms[q], lo, h->kk);
    return RSREC_OK;
}

// the seeds of chains c0 .. c0 + nb - 1 as the kernels take them: 0-based atoms, complex coefficients (1 where the caller gives none)
void stage_seeds(const int32_t* seed_atoms, const double* seed_coef, int c0, int nb, int nseed, std::vector<int>& seeds0, std::vector<double>& coef) {
    const size_t n = (size_t)nb * nseed, g0 = (size_t)c0 * nseed;
    seeds0.resize(n);
    coef.resize(2 * n);
    for (size_t q = 0; q < n; ++q) {
        seeds0[q] = seed_atoms[g0 + q] - 1;
        coef[2 * q] = seed_coef ? seed_coef[2 * (g0 + q)] : 1.0;
        coef[2 * q + 1] = seed_coef ? seed_coef[2 * (g0 + q) + 1] : 0.0;
    }
}

// the side stream and the two events that tie it to the main stream, created when a recursion first runs
int ensure_side_stream(rsrec_t* h) {
    if (h->side_stream) return RSREC_OK;
    HIPCK(h, hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
    HIPCK(h, hipEventCreateWithFlags(&h->ev_orth, hipEventDisableTiming));
    HIPCK(h, hipEventCreateWithFlags(&h->ev_bred, hipEventDisableTiming));
    return RSREC_OK;
}

// Partial sums of a batch of B chains: the first stage as the caller sizes it, the second stage (presum) in two slots -- slot 1 is the side
// stream's -- sized once, never grown mid-stream.  p2_slot decides which reductions take the two-stage path -- their speed, not their rounding:
// the reduce kernels sum partials and presums in the same order (sum_partials16).
int reserve_partials(rsrec_t* h, int B, size_t first_stage_bytes) {
    HIPCK(h, h->d_partial.reserve(first_stage_bytes));
    h->p2_slot = (size_t)B * 16 * 2 * 1296;
    HIPCK(h, h->d_partial2.reserve(2 * h->p2_slot * sizeof(double)));
    return RSREC_OK;
}

// the lists of the region entry upload_regions made current, as the kernels walk them: CV the per-level lists of H|psi>, CVp (where asked
// for) the level-major lists of the streaming passes behind it
void chain_views(const rsrec_t* h, size_t velems, int cpo, ChainView& CV, ChainView* CVp = nullptr) {
    const rsrec_handle::RegionEntry& E = *h->cur_entry;
    const size_t tab = (size_t)E.key.nb * E.key.nlev;
    const int* cum = E.cum.as<int>();
    CV.order = E.order.as<int>(); CV.cum = cum; CV.obase = cum + tab; CV.nlev = E.key.nlev; CV.vstride = velems; CV.cpo = cpo; CV.ostride = E.ostride;
    if (!CVp) return;
    *CVp = CV;
    CVp->cum = cum + 2 * tab; CVp->obase = cum + 3 * tab;
}

// timing of a call from its events: the whole call, the H|psi> kernels (or whatever hop_ev brackets), and the rest
void finish_timing(rsrec_t* h, hipEvent_t ev_begin, hipEvent_t ev_end, const std::vector<std::pair<hipEvent_t, hipEvent_t>>& hop_ev) {
    h->t_total_ms = ev_ms(ev_begin, ev_end);
    for (auto& pr : hop_ev) h->t_hop_ms += ev_ms(pr.first, pr.second);
    h->t_rest_ms = h->t_total_ms - h->t_hop_ms;
}

// end of a call whose kernels report through the status word (cleared when the call began): the word, the stream, the eigen-solver's
// failure (bit 1) or the Chebyshev moments' divergence (bit 2)
int finish_status(rsrec_t* h) {
    int status = 0;
    XFER(xfer_d2h(h, &status, h->d_status.p, 4));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (status & 1) return fail(h, RSREC_ERR_EIG, "Diagonalization error (18x18 Jacobi did not converge)");
    if (status & 2) return fail(h, RSREC_ERR_DIVERGED, "Chebyshev moments did not converge. Check energy limits energy_min and energy_max");
    return RSREC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Workgroups per chain of the matrix-core post-hop kernels (Gram, orthogonalisation, Chebyshev step): they hold their 36x36
// coefficient tables in registers and run one wave per SIMD, so long-lived waves win -- about two workgroups per CU over
// the whole batch (measured at 64 chains: 8 per chain 4.3 ms per level, 64 per chain 5.0 ms).  Three fixed bands, so that the
// work assignment (and with it the rounding of the reductions) only changes when the batch size crosses a band: inside a band a
// chain's bits do not depend on the other chains of the call (a chain of more than 8 x 4 groups in calls of fewer than 32 chains
// and of 32 or more does differ: the cap is another one).
int mfma_workgroups_per_chain(const rsrec_t* h, int batch) {
    if (h->opt_nblk > 0) return (int)std::min<long>(2 * h->opt_nblk, 256);
    return batch >= 32 ? 8 : (batch >= 16 ? 32 : 256);
}

// launch size of a (level) pass: enough workgroups for the largest chain of the batch at that level, at most `full.x`
// (the kernels' own active_workgroups() keeps each chain's work assignment independent of it)
dim3 level_grid(const rsrec_t* h, dim3 full, int level) {
    if (!h->cur_entry || level < 0 || level >= (int)h->cur_entry->level_max.size()) return full;
    const int groups = h->cur_entry->level_max[level] / GROUP;
    return dim3(std::max(1, std::min((int)full.x, (groups + MF_WAVES - 1) / MF_WAVES)), full.y);
}

// k_spmm5 launch: level-sized in x; in y one workgroup per `chain_fold` chains (the kernel loops over them)
// x: one workgroup per 4 groups of the largest chain (not capped at `full.x`): every workgroup then does at most one round of
// groups and the hardware dispatcher balances the CUs; with the 256 cap 10 of the 32 workgroups of an XCD did two rounds
// (measured: folding chains into longer-lived workgroups, i.e. LESS dynamic balancing, costs 10-25 %).
dim3 s5_grid(const rsrec_t* h, dim3 full, int level) {
    int gx = full.x;
    if (h->cur_entry && level >= 0 && level < (int)h->cur_entry->level_max.size()) {
        const int groups = h->cur_entry->level_max[level] / GROUP;
        gx = std::max(1, (groups + S5_WG_GROUPS - 1) / S5_WG_GROUPS);
        if (gx > 8) gx = (gx + 7) / 8 * 8;                 // same number of workgroups on every XCD
        if (h->opt_s5_cap > 0) gx = std::min(gx, (int)h->opt_s5_cap);
    }
    const int fold = (int)std::max<long>(1, h->opt_chain_fold);
    return dim3(gx, (full.y + fold - 1) / fold);
}

// Two-stage reduction of per-workgroup partials (k_presum16): returns the buffer and count the final reduce kernel reads.  `nblk` is the
// launch width, i.e. the LARGEST chain's: whether this stage runs, and either fall-back to the single stage, must not show in any chain's
// result -- the reduce kernels' sum_partials16 is k_presum16's order applied to whatever they read.
const double* presum(rsrec_t* h, const double* partial, int nb, int& nblk, int width, hipStream_t stream = nullptr, int slot = 0) {
    if (nblk <= 32) return partial;
    const int nblk2 = (nblk + 15) / 16;
    const size_t need = (size_t)nb * nblk2 * width;
    if (slot == 0 && h->p2_slot == 0) {
        if (h->d_partial2.reserve(need * sizeof(double)) != hipSuccess) return partial;     // fall back to the single-stage sum
    } else if (need > h->p2_slot) return partial;
    double* out = h->d_partial2.as<double>() + (size_t)slot * h->p2_slot;
    const int nchunk = (width + 255) / 256;
    k_presum16<<<dim3(nblk2 * nchunk, nb), 256, 0, stream ? stream : h->stream>>>(partial, nblk, nblk2, width, out);
    nblk = nblk2;
    return out;
}

// k_spmm5 launch (large launches; CI vectors).  The variant with the operator fragments in LDS serves operators with ONE class of
// atoms (a bulk crystal of one type: every group runs the same stream) whose stream of one spin fits the CU's LDS; per-chain stream
// heads (local-axis runs) keep the global-load variant.
constexpr size_t S5_LDS_LIMIT = 160 * 1024;
// LDS a k_spmm5 workgroup may ask for: what the device grants on request (160 KB on MI355X); asked for once per handle, i.e. per device --
// the attribute is a property of the (function, device) pair, a second handle on another GPU of the process needs its own opt-in
void s5_prepare(rsrec_t* h) {
    if (h->s5_lds_limit != (size_t)-1) return;
    int optin = 0;
    h->s5_lds_limit = 0;
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, h->device) == hipSuccess && optin > 64 * 1024) {
        const int ask = (int)std::min<size_t>((size_t)optin, S5_LDS_LIMIT);
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmm5<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, ask) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmm5<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, ask) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmm5<false, true, false, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, ask) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmm5<false, true, false, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, ask) == hipSuccess &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmm5<true, true, false, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, ask) == hipSuccess)
            h->s5_lds_limit = (size_t)ask;
    }
    (void)hipGetLastError();
}
// one launch: the LDS / persistent form for operator class `one` (>= 0) if it is wanted and fits, else the global-load form
template <bool TWO>
void launch_s5_one(rsrec_t* h, dim3 grid, const SpmmDims& SD, const int* order, const int* cum, const int* iz, const Spmm5Operator& op, int set,
                   const double* in, double* out, const double* in2, const double* extra, int ntau, S5Epilogue epi, int one, S5Gram gram = S5Gram()) {
    const size_t lds_bytes = (size_t)op.ntr * S5_TRIPLE * sizeof(double);
    // s5_lds: 0 never, 1 (default) whenever the groups of the launch are of one class and its stream fits
    const bool want = h->opt_s5_lds >= 1;
    s5_prepare(h);
    const size_t lds_limit = h->s5_lds_limit;
    if (want && one >= 0 && !extra && lds_bytes <= lds_limit) {
        // both output spins on every XCD (workgroup rows alternate between them, an XCD sweeps an eighth of the list) also for collinear
        // operators: the split "even XCDs spin 0, odd XCDs spin 1" of round 2 (an XCD's L2 then holds one spin half of the neighbour blocks)
        // measured 2-4 % slower on every workload at the end of round 3 (tools/ab_spin_xcd.sh); option s5_spin_xcd = 1 brings it back
        const int spin_by_xcd = (op.spin_mixing || !h->opt_s5_spin_xcd) ? 0 : 1;
        const unsigned row = spin_by_xcd ? 8 : 16;
        dim3 g2(std::max(row, (grid.x + row - 1) / row * row), grid.y);
        int* queue = nullptr;
        const unsigned ncu = (unsigned)std::max(16, h->n_cu / 16 * 16);     // whole rows of 8 / 16 workgroups (the kernel's XCD mapping)
        if ((h->opt_s5_queue == 1 && grid.x >= ncu) || h->opt_s5_queue >= 2) {
            // persistent form: one workgroup per CU for the whole launch, groups from per-(chain, XCD[, spin]) counters
            if ((!h->capturing || h->d_s5queue.bytes >= (size_t)SD.nchains * 16 * sizeof(int)) &&     // (no allocation inside a stream capture)
                h->d_s5queue.reserve((size_t)SD.nchains * 16 * sizeof(int)) == hipSuccess &&
                hipMemsetAsync(h->d_s5queue.p, 0, (size_t)SD.nchains * 16 * sizeof(int), h->stream) == hipSuccess) {
                queue = h->d_s5queue.as<int>();
                g2 = dim3(ncu, 1);
            }
        }
        // s5_waves = 4 (persistent form only): half-size workgroups, one wave per SIMD -- the other half of every CU's registers stays free
        // for the kernels of another stream (the HBM-bound post-hop passes of the other half batch)
        const unsigned thr = (queue && h->opt_s5_waves == 4) ? S5_WG_GROUPS * 64 : S5_WG_GROUPS * 128;
        if (queue && h->opt_s5_split == 3) {
            const unsigned thr3 = 64u * (unsigned)std::min<long>(12, std::max<long>(8, h->opt_s5_waves));       // (launch bounds: 768 threads)
            // the split stream requests its operands five steps ahead: up to two triples past the stream's end (never used) -- one more triple of LDS where it fits
            const size_t lds3 = std::min(lds_limit, lds_bytes + (size_t)S5_TRIPLE_BYTES);
            k_spmm5<TWO, true, false, 3><<<g2, thr3, lds3, h->stream>>>(SD, order, cum, h->d_nbr5.as<int>(), iz, op.frag_set(set), op.meta_set(set), op.ntr, in, out, in2, nullptr, ntau, one, queue, spin_by_xcd, epi);
        } else if constexpr (!TWO) {
            if (gram.out) k_spmm5<false, true, false, 1, true><<<g2, thr, lds_bytes, h->stream>>>(SD, order, cum, h->d_nbr5.as<int>(), iz, op.frag_set(set), op.meta_set(set), op.ntr, in, out, in2, nullptr, ntau, one, queue, spin_by_xcd, epi, gram);
            else k_spmm5<false, true><<<g2, thr, lds_bytes, h->stream>>>(SD, order, cum, h->d_nbr5.as<int>(), iz, op.frag_set(set), op.meta_set(set), op.ntr, in, out, in2, nullptr, ntau, one, queue, spin_by_xcd, epi);
        } else
        k_spmm5<TWO, true><<<g2, thr, lds_bytes, h->stream>>>(SD, order, cum, h->d_nbr5.as<int>(), iz, op.frag_set(set), op.meta_set(set), op.ntr, in, out, in2, nullptr, ntau, one, queue, spin_by_xcd, epi);
    } else if constexpr (!TWO) {
        if (gram.out) k_spmm5<false, false, false, 1, true><<<grid, S5_WG_GROUPS * 128, 0, h->stream>>>(SD, order, cum, h->d_nbr5.as<int>(), iz, op.frag_set(set), op.meta_set(set), op.ntr, in, out, in2, extra, ntau, 0, nullptr, 1, epi, gram);
        else k_spmm5<false, false><<<grid, S5_WG_GROUPS * 128, 0, h->stream>>>(SD, order, cum, h->d_nbr5.as<int>(), iz, op.frag_set(set), op.meta_set(set), op.ntr, in, out, in2, extra, ntau, 0, nullptr, 1, epi);
    } else
        k_spmm5<TWO, false><<<grid, S5_WG_GROUPS * 128, 0, h->stream>>>(SD, order, cum, h->d_nbr5.as<int>(), iz, op.frag_set(set), op.meta_set(set), op.ntr, in, out, in2, extra, ntau, 0, nullptr, 1, epi);
}

// k_spmm5 launch (CI vectors).  The operator fragments sit in LDS (one copy per persistent workgroup) when all groups a workgroup takes
// run the same stream: operators with ONE class of atoms (a bulk crystal of one type).  Operators with several classes (surfaces,
// compounds, impurity clusters) can take the same form per LARGE CLASS RUN of the class-sorted list of all atoms -- the list every chain
// uses once its region covers the lattice: one persistent launch whose workgroup rows are dealt to the runs, plus one global-load launch
// for what remains (small classes such as the per-atom blocks of an impurity region, chains whose regions are still growing) -- option
// s5_lds = 2; by default they keep the global-load form, which is faster for them.  Per-chain stream heads (local-axis runs): global loads.
template <bool TWO>
void launch_s5(rsrec_t* h, dim3 grid, const SpmmDims& SD0, const int* order, const int* cum, const int* iz, const Spmm5Operator& op, int set,
               const double* in, double* out, const double* in2 = nullptr, const double* extra = nullptr, int ntau = 0, S5Epilogue epi = S5Epilogue(),
               S5Gram gram = S5Gram() /*the caller established that the operator is one the Gram fold serves (gram_eligible)*/) {
    SpmmDims SD = SD0;
    const int one = op.single_class(set);
    const rsrec_handle::RegionEntry* E = h->cur_entry;
    // s5_lds = 2: the class-run form (measured slower than the global-load form on both multi-class workloads of bench.py -- fccCu001
    // 5.58 vs 5.25 ms per launch, and the launch-per-run variant B2FeCo 3.07 vs 2.36 ms: the runs cannot balance against each other --
    // so it is not the default; the parity tests run it)
    const bool multi = one < 0 && h->opt_s5_lds >= 2 && !extra && E && E->sat_base > 0 && SD.cpo == 1 && SD.level >= 0 && SD.level < (int)E->level_sat.size() &&
                       E->level_sat[SD.level] > 0 && op.ntau == h->nmax + h->ntype && (grid.x >= (unsigned)std::max(16, h->n_cu / 16 * 16) || h->opt_s5_queue >= 2) && (size_t)op.ntr * S5_TRIPLE * sizeof(double) <= (s5_prepare(h), h->s5_lds_limit);
    // Atoms with their own operator blocks (an impurity region: classes 0 .. nmax - 1) are one-tile groups of their own in a chain's lists.
    // From `s5_octet` such atoms on, and once at least half of the (atom, chain) pairs of the batch are inside their chains' regions, a
    // launch of its own forms their groups over 8 CHAINS instead -- the chains share the atom's fragments; an atom outside a chain's
    // region has no active neighbour there and comes out as the zeros it already is -- and the main launch passes over them.
    bool octets = false, oct_aside = false;
    double pa_pairs = 0.0;
    if (E && SD.level >= 0 && (size_t)(SD.level + 1) * op.ntau <= E->level_groups.size() && op.ntau == h->nmax + h->ntype)
        for (int t = 0; t < h->nmax; ++t) pa_pairs += E->level_groups[(size_t)SD.level * op.ntau + t];
    if (!multi && one < 0 && h->opt_s5_octet > 0 && h->nmax >= h->opt_s5_octet && !extra && E && SD.cpo == 1 && SD.nchains >= 2 && op.ntau == h->nmax + h->ntype &&
        2.0 * pa_pairs >= (double)h->nmax * SD.nchains && (double)GROUP * (double)(h->kk + 1) * BLD * 8.0 < 4294967296.0) {
        SpmmDims SO = SD;
        const dim3 go((unsigned)((h->nmax + S5_WG_GROUPS - 1) / S5_WG_GROUPS), (unsigned)((SD.nchains + GROUP - 1) / GROUP));
        // beside the main launch, on a stream of its own (the two write disjoint blocks of `out`): alone it is a launch of a few hundred
        // groups with the whole GPU to itself
        hipStream_t so = h->stream;
        if (h->opt_side && !h->oct_stream && !h->capturing &&
            (hipStreamCreateWithFlags(&h->oct_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&h->ev_oct_in, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&h->ev_oct_out, hipEventDisableTiming) != hipSuccess)) { h->oct_stream = nullptr; (void)hipGetLastError(); }
        if (h->opt_side && h->oct_stream && h->ev_oct_in && h->ev_oct_out && hipEventRecord(h->ev_oct_in, h->stream) == hipSuccess &&
            hipStreamWaitEvent(h->oct_stream, h->ev_oct_in, 0) == hipSuccess) { so = h->oct_stream; oct_aside = true; }
        k_spmm5<TWO, false, true><<<go, S5_WG_GROUPS * 128, 0, so>>>(SO, order, cum, h->d_nbr5.as<int>(), iz, op.frag_set(set), op.meta_set(set), op.ntr, in, out, in2, nullptr, ntau,
                                                                   0, nullptr, 1, epi);
        if (oct_aside) (void)hipEventRecord(h->ev_oct_out, h->oct_stream);
        const bool all_sat = E->sat_base > 0 && SD.level < (int)E->level_sat.size() && E->level_sat[SD.level] == SD.nchains && (int)E->sat_runs.size() >= h->nmax &&
                             E->sat_runs[0].tau == 0 && E->sat_runs[0].lo == 0 && E->sat_runs[h->nmax - 1].tau == h->nmax - 1 && E->sat_runs[h->nmax - 1].hi == h->nmax;
        if (all_sat) {
            // every chain is on the class-sorted list of all atoms, whose first nmax groups are those atoms: the main launch takes the rest
            // of that list as ONE run, so that its XCD chunks are cut from what it serves
            SD.sat_base = E->sat_base; SD.run_lo = h->nmax; SD.run_hi = E->sat_runs.back().hi;
        } else SD.skip_pa = 1;
        octets = true;
        h->n_octet_launch++;
    }
    if (!multi) {
        launch_s5_one<TWO>(h, grid, SD, order, cum, iz, op, set, in, out, in2, extra, ntau, epi, one, gram);
        if (oct_aside) (void)hipStreamWaitEvent(h->stream, h->ev_oct_out, 0);            // the level goes on when both launches are done
    } else {
        // class runs worth workgroups of their own: at least two groups per workgroup of a full persistent launch over the chains on the list
        SD.sat_base = E->sat_base;
        const long min_groups = h->opt_s5_run_min > 0 ? h->opt_s5_run_min : std::max<long>(64, 2L * h->n_cu * 8 / std::max(1, E->level_sat[SD.level]));
        const int spin_by_xcd = op.spin_mixing ? 0 : 1;
        const int row = spin_by_xcd ? 8 : 16;
        const int ncu = std::max(16, h->n_cu / 16 * 16), total_rows = ncu / row;
        SpmmDims SR = SD;
        long sum_groups = 0;
        for (const auto& R : E->sat_runs) {
            if (SR.nruns == 4 || R.hi - R.lo < min_groups || op.ksteps[(size_t)set * op.ntau + R.tau] == 0) continue;
            SR.run_tau[SR.nruns] = R.tau; SR.run_glo[SR.nruns] = R.lo; SR.run_ghi[SR.nruns] = R.hi; ++SR.nruns;
            sum_groups += R.hi - R.lo;
        }
        const size_t qbytes = (size_t)4 * SD.nchains * 16 * sizeof(int);
        const bool can = SR.nruns > 0 && SR.nruns <= total_rows && (h->opt_s5_queue >= 1) && (!h->capturing || h->d_s5queue.bytes >= qbytes) &&
                         h->d_s5queue.reserve(qbytes) == hipSuccess && hipMemsetAsync(h->d_s5queue.p, 0, qbytes, h->stream) == hipSuccess;
        if (can) {
            // ONE persistent launch: the workgroup rows are dealt to the runs in proportion to their groups (at least one row each), every
            // run with its own counters; the launch-per-run form paid one tail per run (measured: B2FeCo 22 %, fccCu001 5 % slower)
            int left = total_rows - SR.nruns, acc = 0;
            for (int r = 0; r < SR.nruns; ++r) {
                const long gr = SR.run_ghi[r] - SR.run_glo[r];
                int extra_rows = r == SR.nruns - 1 ? left : (int)std::min<long>(left, (gr * (total_rows - SR.nruns) + sum_groups / 2) / std::max(1L, sum_groups));
                left -= extra_rows;
                SR.run_row0[r] = acc;
                acc += 1 + extra_rows;
            }
            SR.run_row0[SR.nruns] = acc;
            const size_t lds_bytes = (size_t)op.ntr * S5_TRIPLE * sizeof(double);
            k_spmm5<TWO, true><<<dim3(ncu, 1), S5_WG_GROUPS * 128, lds_bytes, h->stream>>>(SR, order, cum, h->d_nbr5.as<int>(), iz, op.frag_set(set), op.meta_set(set), op.ntr, in, out, in2, nullptr, ntau,
                                                                                          0, h->d_s5queue.as<int>(), spin_by_xcd, epi);
            for (int r = 0; r < SR.nruns; ++r) { SD.skip_lo[r] = SR.run_glo[r]; SD.skip_hi[r] = SR.run_ghi[r]; }
            SD.nskip = SR.nruns;
        }
        launch_s5_one<TWO>(h, grid, SD, order, cum, iz, op, set, in, out, in2, nullptr, ntau, epi, -1);
    }
    if (E && SD.level >= 0 && (size_t)(SD.level + 1) * op.ntau <= E->level_groups.size() && SD.cpo == 1 && op.ntau == h->nmax + h->ntype)
        for (int t = 0; t < op.ntau; ++t) {
            double groups = E->level_groups[(size_t)SD.level * op.ntau + t];
            if (octets && t < h->nmax) groups = (double)((SD.nchains + GROUP - 1) / GROUP);          // one group per octet of chains instead of one per chain
            h->n_hop_mfma_flop += groups * op.flops_per_group(set, t);
        }
}

// k_spmm4 addresses a chain's vector with 32-bit byte offsets: only below 4 GiB per chain vector (828 000 atoms)
bool spmm4_usable(const rsrec_t* h) { return h->s5_built && !h->hoh && (size_t)(h->kk + 1) * BLD * sizeof(double) < ((size_t)1 << 32); }

// k_spmm4's fragment tables of the operator as last set (plain operator only: hoh calls always take k_spmm5), built on first use
int ensure_s4(rsrec_t* h) {
    if (h->s4_built_split) return RSREC_OK;
    const char* msg = h->s4_op.build(h->nslots, h->hslots, h->ntype, h->nmax, 0, h->host_st.data(), h->nmax > 0 ? h->host_loc.data() : nullptr, nullptr, nullptr, 1);
    if (msg) return fail(h, RSREC_ERR_DEVICE, "k_spmm4 operator tables: %s", msg);
    h->s4_built_split = 1;
    return RSREC_OK;
}

// small-launch SpMM on LayoutRM vectors: out = sum_slots H_slot in_nbr, four waves share one group of atoms (k_spmm4<4>)
int s4_prepare(rsrec_t* h) {
    if (!h->s4_attr) {
        HIPCK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_spmm4<4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)S4_LDS_BYTES));
        h->s4_attr = true;
    }
    return RSREC_OK;
}
int launch_spmm(rsrec_t* h, const SpmmDims& SD, const ChainView& CV, const DevProblem& P, int set, const double* in, double* out, dim3 grid_mf) {
    { const int rc = s4_prepare(h); if (rc) return rc; }
    // one group per workgroup at a time: 4x as many workgroups keep the same number of groups in flight per launch
    dim3 g4(std::min<unsigned>(grid_mf.x * 4, 1024), grid_mf.y);
    k_spmm4<4><<<g4, MF_WAVES * 64, S4_LDS_BYTES, h->stream>>>(SD, CV.order, CV.cum, P.nbr, P.iz, h->s4_op.frag_set(set), h->s4_op.meta_set(set), in, out);
    return RSREC_OK;
}

// Local-axis runs: the resident coefficients of chain s into the spin frame of its site, M <- R_s^H (M R_s) in place, for every matrix
// the reference's chain leaves general: a_b of levels 1 .. lld - 1 and b2_b of levels 2 .. lld (a_b(:,:,lld) = 0 and b2_b(:,:,1) = I stay
// exact, recursion.f90:1836-1837).  One workgroup per matrix: blockIdx.x < lld - 1 is a_b at level blockIdx.x, the others b2_b one level up.
// Both 18-term sums run k ascending, every term ar*br - ai*bi / ar*bi + ai*br rounded before it is added, no FMA contraction: the bits of
// the same loops on a host without FMA.  M, R: column-major 18 x 18.
__global__ __launch_bounds__(256) void k_rotate_coef(double2* __restrict__ A, double2* __restrict__ B, const double2* __restrict__ rot, int lld) {
#pragma clang fp contract(off)
    __shared__ double2 sM[BLK], sR[BLK], sT[BLK];
    const int chain = blockIdx.y, m = blockIdx.x;
    const bool is_a = m < lld - 1;
    double2* M = (is_a ? A : B) + ((size_t)chain * lld + (is_a ? m : m - (lld - 1) + 1)) * BLK;
    const double2* R = rot + (size_t)chain * BLK;
    for (int e = threadIdx.x; e < BLK; e += blockDim.x) { sM[e] = M[e]; sR[e] = R[e]; }
    __syncthreads();
    for (int e = threadIdx.x; e < BLK; e += blockDim.x) {            // T = M R
        const int i = e % NB, j = e / NB;
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const double ar = sM[i + NB * k].x, ai = sM[i + NB * k].y, br = sR[k + NB * j].x, bi = sR[k + NB * j].y;
            sr += ar * br - ai * bi; si += ar * bi + ai * br;
        }
        sT[e] = make_double2(sr, si);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < BLK; e += blockDim.x) {            // M = R^H T
        const int i = e % NB, j = e / NB;
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const double ar = sR[k + NB * i].x, ai = -sR[k + NB * i].y, br = sT[k + NB * j].x, bi = sT[k + NB * j].y;
            sr += ar * br - ai * bi; si += ar * bi + ai * br;
        }
        M[e] = make_double2(sr, si);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// What the chain drivers (run_block_lanczos, run_chebyshev, run_pairs_direct, run_bloch) share, as the pair calls share PairCall and the on-site
// stages SiteStage: the call's decisions and reservations (RecursionCall), a batch's uploads (RecursionBatch), seed_chains, the H|psi> step of
// either kernel set (apply_h, valu_apply_h), SideReduce and replay_level_loop; the Chebyshev drivers also the three-term recurrence
// (ChainChebyshev), and the two "one chain per atom" drivers their whole level loop (chain_level_loop).
struct RecursionCall {
    bool mfma = false, side = false;     // kernel set; the side stream takes the levels' reductions
    int nchains = 0, nseed = 1, napply = 0, nlev = 0;   // napply: applications of H per chain; nlev: levels of its region lists
    const double* rot = nullptr;         // local-axis runs: complex (18,18,nchains), the spin-frame rotation of every chain
    const Spmm5Operator* op = nullptr;   // what k_spmm5 applies (local-axis runs: H without the on-site l.s term)
    int ci = 0;                          // 1: CI vectors and k_spmm5; 0: LayoutRM with k_spmm4, or LayoutCM with the VALU set
    size_t velems = 0;                   // doubles per chain per vector (+1: the all-zero block)
    int nvec = 0, skip_vec = -1, B = 1, nblk = 1;   // (recursion_begin) work vectors -- skip_vec is neither allocated nor cleared --, batch, workgroups
    DevProblem P;
    hipEvent_t ev_begin = nullptr;       // start of the timed span
    std::vector<std::pair<hipEvent_t, hipEvent_t>> hop_ev, rot_ev;   // H|psi> of every step; k_rotate_coef of every batch
};

// Matrix-core set: k_spmm5 with every vector in the CI layout (option spmm5 = 2, the default since round 3: with the operator
// streams assembled on the device a call no longer pays k_spmm4's host swizzle -- 3 ms per SCF iteration on the 18 operator classes
// of B2FeCo, tools/time_set_hamiltonian.py -- and k_spmm5 is as fast on one chain).  spmm5 = 1: small launches of the plain operator
// take the cooperative k_spmm4<4> on LayoutRM (kept as the cross-check of the parity tests); 0: k_spmm4 whenever it can.  hoh and
// local-axis (rot) calls always take k_spmm5.
RecursionCall recursion_call(const rsrec_t* h, bool mfma, int nchains, int nseed, int napply, const double* rot = nullptr) {
    RecursionCall RC;
    RC.mfma = mfma; RC.nchains = nchains; RC.nseed = nseed; RC.napply = napply; RC.rot = rot;
    RC.nlev = (h->hoh ? 2 * napply : napply) + 1; RC.op = rot ? &h->s5_la : &h->s5_op; RC.velems = (size_t)(h->kk + 1) * BLD;
    const bool large = (long)std::min(nchains, 64) * (h->kk / GROUP + 1) >= 4096;
    RC.ci = (mfma && (h->hoh || rot || h->opt_spmm5 == 2 || (h->opt_spmm5 == 1 && large) || !spmm4_usable(h))) ? 1 : 0;
    return RC;
}

// kernels: 0 = auto, 1 = FP64 VALU kernel set, 2 = matrix-core set.  The matrix-core SpMM tables exist for lattices with up to
// S4_MAXSLOTS - 1 neighbour slots; beyond that the VALU set (any stencil) runs.
bool matrix_core_set(const rsrec_t* h) { return h->opt_kernels != 1 && h->s5_built; }
// what the last call left resident is gone once a call reserves (or overwrites) the buffers it lay in
void drop_resident(rsrec_t* h) { h->res_kind = 0; h->spec_res.nop = 0; }

// Plans the batches and reserves what every recursion needs: `nvec` work vectors (all but `skip_vec`), the partials, the seeds with `coef_slots`
// coefficients per chain, the status word (cleared here), the side stream; opens the timed span.  The caller reserves its resident outputs BEFORE it.
int recursion_begin(rsrec_t* h, RecursionCall& RC, int nvec, int skip_vec, int coef_slots, size_t gram_doubles_per_chain = 0) {
    if (RC.mfma && !RC.ci) XFER(ensure_s4(h));
    RC.nvec = nvec; RC.skip_vec = skip_vec;
    BatchPlan bp;
    XFER(plan_batch(h, RC.nchains, nvec - (skip_vec >= 0 ? 1 : 0), RC.velems / 2, bp, gram_doubles_per_chain * sizeof(double)));
    const int B = RC.B = bp.batch; RC.nblk = bp.nblk;
    for (int v = 0; v < nvec; ++v) if (v != skip_vec) HIPCK(h, h->d_vec[v].reserve((size_t)B * RC.velems * sizeof(double)));
    // the folded Gram's partials go with the work vectors: reserved here, before any stream capture
    if (gram_doubles_per_chain) HIPCK(h, h->d_gram.reserve((size_t)B * gram_doubles_per_chain * sizeof(double)));
    // first stage: two Gram partials (1296 doubles) of up to 256 workgroups per chain; the VALU set's 2 nblk <= 512 partials are as large
    XFER(reserve_partials(h, B, (size_t)B * 256 * 2 * 1296 * sizeof(double)));
    XFER(ensure_side_stream(h));
    RC.side = h->opt_side && h->side_stream;
    if (RC.rot) HIPCK(h, h->d_la_extra.reserve((size_t)B * (h->nmax + h->ntype) * S5_HEAD_DOUBLES * sizeof(double)));
    HIPCK(h, h->d_status.reserve(64));
    HIPCK(h, h->d_seed.reserve((size_t)B * RC.nseed * 4));
    HIPCK(h, h->d_seedcoef.reserve((size_t)B * coef_slots * sizeof(double2)));
    HIPCK(h, hipMemsetAsync(h->d_status.p, 0, 64, h->stream));
    RC.P = make_problem(h); RC.ev_begin = next_event(h);
    return RSREC_OK;
}

// local-axis runs: the on-site term of chains c0 .. c0 + nb - 1 in the GLOBAL frame, (e_nu +) R l.s R^H, as k_spmm5's stream heads (see rsrec_block_lanczos_local_axis)
void local_axis_fragments(const rsrec_t* h, const Spmm5Operator& OP, const double* rot, int c0, int nb, std::vector<double>& fr) {
    const bool hoh = h->hoh != 0;
    const int ntau = h->nmax + h->ntype, la_fps = S5_HEAD_DOUBLES;
    std::vector<double> E(2 * BLK), T(2 * BLK); fr.assign((size_t)nb * ntau * la_fps, 0.0);
    for (int c = 0; c < nb; ++c) {
        const double* R = rot + 2 * (size_t)BLK * (c0 + c);
        for (int tau = 0; tau < ntau; ++tau) {
            const int ty = tau < h->nmax ? h->iz0[tau] : tau - h->nmax;
            const double* ls = h->host_lsham.data() + 2 * (size_t)BLK * ty;
            for (int j = 0; j < NB; ++j)                    // T = l.s R^H
                for (int i = 0; i < NB; ++i) {
                    double sr = 0.0, si = 0.0;
                    for (int k = 0; k < NB; ++k) {
                        const double ar = ls[2 * (i + NB * k)], ai = ls[2 * (i + NB * k) + 1], br = R[2 * (j + NB * k)], bi = -R[2 * (j + NB * k) + 1];
                        sr += ar * br - ai * bi; si += ar * bi + ai * br;
                    }
                    T[2 * (i + NB * j)] = sr; T[2 * (i + NB * j) + 1] = si;
                }
            for (int j = 0; j < NB; ++j)                    // E = R T
                for (int i = 0; i < NB; ++i) {
                    double sr = 0.0, si = 0.0;
                    for (int k = 0; k < NB; ++k) {
                        const double ar = R[2 * (i + NB * k)], ai = R[2 * (i + NB * k) + 1], br = T[2 * (k + NB * j)], bi = T[2 * (k + NB * j) + 1];
                        sr += ar * br - ai * bi; si += ar * bi + ai * br;
                    }
                    E[2 * (i + NB * j)] = sr; E[2 * (i + NB * j) + 1] = si;
                }
            if (hoh) for (int e = 0; e < 2 * BLK; ++e) E[e] += h->host_enim[2 * (size_t)BLK * ty + e];
            OP.emit_head(hoh ? 1 : 0, tau, E.data(), fr.data() + ((size_t)c * ntau + tau) * la_fps);
        }
    }
}

struct RecursionBatch {                  // what the level loop of one batch works on
    int nb = 0, ostride = 0;
    ChainView CV, CVp;                   // CVp: the streaming passes walk the level-major lists (upload_regions)
    dim3 grid_mf;                        // launch of the matrix-core passes: workgroups per chain x chains
    const double* la_extra = nullptr;    // local-axis runs: the chains' on-site fragments (d_la_extra)
};
// Per-batch prologue of chains c0 .. c0 + nb - 1: seeds, regions (cached) and, in a local-axis run, the on-site fragments go to the device;
// returns when they are there.  `extra_coef` may append to the staged coefficients before they are uploaded.  All of it is host time.
using SeedCoefHook = void (*)(int nb, int nseed, const std::vector<int>& seeds0, std::vector<double>& coef);
int recursion_batch(rsrec_t* h, const RecursionCall& RC, const int32_t* seed_atoms, const double* seed_coef, int c0, int nb, RecursionBatch& b,
                    SeedCoefHook extra_coef = nullptr) {
    const auto th0 = std::chrono::steady_clock::now();
    std::vector<int> seeds0;
    std::vector<double> coef, fr;
    stage_seeds(seed_atoms, seed_coef, c0, nb, RC.nseed, seeds0, coef);
    if (extra_coef) extra_coef(nb, RC.nseed, seeds0, coef);
    XFER(upload_regions(h, seeds0.data(), nb, RC.nseed, RC.nlev, RC.napply, h->hoh != 0, RC.mfma));
    b.nb = nb; b.ostride = h->cur_entry->ostride;
    h->n_atom_steps += h->cur_entry->atom_steps; h->n_block_mult += h->cur_entry->block_mults;
    h->n_req_flop += required_hop_flops(h, *RC.op);
    XFER(xfer_h2d(h, h->d_seed.p, seeds0.data(), seeds0.size() * 4));
    XFER(xfer_h2d(h, h->d_seedcoef.p, coef.data(), coef.size() * 8));
    if (RC.rot) {
        local_axis_fragments(h, *RC.op, RC.rot, c0, nb, fr);
        XFER(xfer_h2d(h, h->d_la_extra.p, fr.data(), fr.size() * sizeof(double)));
        b.la_extra = h->d_la_extra.as<double>();
    }
    HIPCK(h, hipStreamSynchronize(h->stream));
    h->t_host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count();
    chain_views(h, RC.velems, 1, b.CV, &b.CVp);
    b.grid_mf = dim3(std::max(1, std::min(mfma_workgroups_per_chain(h, RC.B), (b.ostride / GROUP + MF_WAVES - 1) / MF_WAVES)), nb);
    return RSREC_OK;
}

// clears the work vectors of a batch; of vector `zero_block_only` (-1: none) only the zero block kk (one 2-D memset over the chains)
int clear_vectors(rsrec_t* h, const RecursionCall& RC, int nb, int zero_block_only = -1) {
    for (int v = 0; v < RC.nvec; ++v) {
        if (v == RC.skip_vec) continue;
        if (v == zero_block_only)
            HIPCK(h, hipMemset2DAsync(static_cast<char*>(h->d_vec[v].p) + (size_t)h->kk * BLD * sizeof(double), RC.velems * sizeof(double), 0, BLD * sizeof(double), (size_t)nb, h->stream));
        else HIPCK(h, hipMemsetAsync(h->d_vec[v].p, 0, (size_t)nb * RC.velems * sizeof(double), h->stream));
    }
    return RSREC_OK;
}
// One H|psi> of the matrix-core set, dst = H src, as application `step` (1, 2, ...) of the batch's chains, between the events the call's hop
// time is read from.  k_spmm5 on CI vectors: one launch, or with hoh two -- h src into `hps` on the lists of level 2 step - 1, then
// H = h - (h o) h + e_nu + l.s with src as second input (extra on-site slot) on those of level 2 step.  `extra` / `ntau`: the per-chain on-site
// fragments of a local-axis run (the single launch is then a two-input one as well).  Else the cooperative k_spmm4 on LayoutRM (plain operator).
int apply_h(rsrec_t* h, RecursionCall& RC, const RecursionBatch& b, int step, const double* src, double* dst, double* hps, const double* extra, int ntau,
            S5Epilogue epi = S5Epilogue(), S5Gram gram = S5Gram()) {
    const bool hoh = h->hoh != 0;
    const int lv_final = hoh ? 2 * step : step;
    const Spmm5Operator& OP = *RC.op; const DevProblem& P = RC.P; const ChainView& CV = b.CV;
    hipEvent_t e0 = next_event(h);                   // [e0, e1] brackets exactly the H|psi> kernel(s) of this step
    SpmmDims SD{h->kk, P.nslots, P.nmax, RC.nlev, 1, b.ostride, hoh ? 2 * step - 1 : lv_final, RC.velems, CV.obase, b.nb};
    if (!RC.ci) XFER(launch_spmm(h, SD, CV, P, 0, src, dst, b.grid_mf));
    else if (hoh) {
        launch_s5<false>(h, s5_grid(h, b.grid_mf, 2 * step - 1), SD, CV.order, CV.cum, P.iz, OP, 0, src, hps);
        SD.level = lv_final;
        launch_s5<true>(h, s5_grid(h, b.grid_mf, lv_final), SD, CV.order, CV.cum, P.iz, OP, 1, hps, dst, src, extra, ntau, epi);
    } else if (extra) launch_s5<true>(h, s5_grid(h, b.grid_mf, lv_final), SD, CV.order, CV.cum, P.iz, OP, 0, src, dst, src, extra, ntau, epi);
    else launch_s5<false>(h, s5_grid(h, b.grid_mf, lv_final), SD, CV.order, CV.cum, P.iz, OP, 0, src, dst, nullptr, nullptr, 0, epi, gram);
    RC.hop_ev.emplace_back(e0, next_event(h)); h->n_hop_launch += hoh ? 2 : 1;
    return RSREC_OK;
}

// the Chebyshev step as the epilogue of the launch that forms H cur:  out = (H cur - b cur)/a  [* 2 - old]
S5Epilogue cheb_epilogue(bool first, const double* cur, const double* old, double a, double b) {
    S5Epilogue E; E.kind = first ? 1 : 2; E.cur = cur; E.old = first ? nullptr : old; E.a = a; E.b = b;
    return E;
}
// One H|psi> of the VALU set (LayoutCM), the counterpart of apply_h: `out` = MODE of H src as application `step` of the batch's chains, between
// the events the call's hop time is read from.  With hoh two launches -- h src into `hps` on the lists of level 2 step - 1, then MODE_HOH on
// those of level 2 step.  v0: psi (Lanczos) | T_{n-2} (Chebyshev); ca, cb: the Chebyshev scaling.  The Gram partials go to d_partial.
template <int MODE, int MODE_HOH>
int valu_apply_h(rsrec_t* h, RecursionCall& RC, const RecursionBatch& b, int step, const double* src, const double* v0, double* out, double* hps,
                 double ca = 0.0, double cb = 0.0) {
    const bool hoh = h->hoh != 0;
    const dim3 grid(RC.nblk, b.nb);
    hipEvent_t e0 = next_event(h);                   // [e0, e1] brackets exactly the H|psi> kernel(s) of this step
    ApplyArgs G{};
    G.partial = h->d_partial.as<double2>(); G.a = ca; G.b = cb; G.in = src; G.cur = src; G.v0 = v0; G.out = out; G.level = step;
    if (!hoh) k_apply<MODE, LayoutCM><<<grid, NTHREADS, 0, h->stream>>>(RC.P, b.CV, G);
    else {
        G.out = hps; G.level = 2 * step - 1;
        k_apply<AM_STORE, LayoutCM><<<grid, NTHREADS, 0, h->stream>>>(RC.P, b.CV, G);
        G.in = hps; G.v1 = hps; G.out = out; G.level = 2 * step;
        k_apply<MODE_HOH, LayoutCM><<<grid, NTHREADS, 0, h->stream>>>(RC.P, b.CV, G);
    }
    RC.hop_ev.emplace_back(e0, next_event(h)); h->n_hop_launch += hoh ? 2 : 1;
    return RSREC_OK;
}

// k_seed on vector `vec` of a batch's chains, in the layout the call's kernels read: CI (k_spmm5), LayoutRM (k_spmm4) or LayoutCM (VALU set)
void seed_chains(rsrec_t* h, const RecursionCall& RC, int nb, double* vec) {
    const auto seed = RC.ci ? k_seed<LayoutCI> : RC.mfma ? k_seed<LayoutRM> : k_seed<LayoutCM>;
    seed<<<nb, 64, 0, h->stream>>>(vec, RC.velems, h->d_seed.as<int>(), h->d_seedcoef.as<double2>(), RC.nseed);
}

// The three-term recurrence on a batch's chains, H~ = (H - b)/a, shaped like ChebyshevStepper: with T_0(H~) x in `cur` (work vector 0),
// step(t) for t = 1, 2, ... leaves T_t(H~) x in `cur`, T_{t-1}(H~) x in `old` and the region level it ran on in `level`; from t = 2 on work
// vectors 0 .. 2 rotate, and `spare` is T_{t-2}(H~) x.  VALU set: k_apply forms `cur` (tmp: h psi of the hoh first pass).  Matrix-core set:
// k_spmm5's epilogue forms it (hps: h psi of the hoh first pass) -- or, with `plain_h`, apply_h leaves H old in `tmp` and the caller forms `cur`
// (run_chebyshev with cheb_fused = 0, and k_spmm4, which has no epilogue).
struct ChainChebyshev {
    double *old, *cur, *spare, *tmp, *hps;
    double a, b;
    int level = 0;
    ChainChebyshev(const rsrec_t* h, const RecursionCall& RC, double a_, double b_)
        : old(h->d_vec[1].as<double>()), cur(h->d_vec[0].as<double>()), spare(h->d_vec[2].as<double>()), tmp(h->d_vec[3].as<double>()),
          hps(RC.ci && h->hoh ? h->d_vec[4].as<double>() : nullptr), a(a_), b(b_) {}
    int step(rsrec_t* h, RecursionCall& RC, const RecursionBatch& bt, int t, bool plain_h = false) {
        const bool first = t == 1;
        if (first) std::swap(old, cur);
        else { double* o = spare; spare = old; old = cur; cur = o; }
        level = h->hoh ? 2 * t : t;
        if (RC.mfma) return apply_h(h, RC, bt, t, old, plain_h ? tmp : cur, hps, nullptr, 0, plain_h ? S5Epilogue() : cheb_epilogue(first, old, spare, a, b));
        if (first) return valu_apply_h<AM_CHEB1, AM_HOH_CHEB1>(h, RC, bt, t, old, old, cur, tmp, a, b);
        return valu_apply_h<AM_CHEBN, AM_HOH_CHEBN>(h, RC, bt, t, old, spare, cur, tmp, a, b);
    }
};

// The level loop of the "one chain per atom" drivers on one batch: clear, seed, then the vector of every order n = 0 .. napply goes to
// pass(vec, region level, n) as soon as it is formed; returns when the stream is idle (the next batch's uploads reuse the seeds).
template <class Pass>
int chain_level_loop(rsrec_t* h, RecursionCall& RC, const RecursionBatch& bt, double a, double b, Pass&& pass) {
    XFER(clear_vectors(h, RC, bt.nb));
    ChainChebyshev S(h, RC, a, b);
    seed_chains(h, RC, bt.nb, S.cur);
    pass(S.cur, 0, 0);
    for (int t = 1; t <= RC.napply; ++t) {
        XFER(S.step(h, RC, bt, t));
        pass(S.cur, S.level, t);
    }
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(h->stream));
    return RSREC_OK;
}
// The side-stream hand-off of a level's reduction (partial sums -> coefficients), which the main stream's next H|psi> does not need: begin
// gives the stream to reduce on -- with `side` the side stream, behind everything queued on the main stream so far --, end marks the
// reduction's end there, and wait holds the main stream until then: before the first launch that reads its result or reuses its input.
struct SideReduce { bool side = false, pending = false; };
int side_reduce_begin(rsrec_t* h, const SideReduce& S, hipStream_t& st) {
    st = S.side ? h->side_stream : h->stream;
    if (S.side) { HIPCK(h, hipEventRecord(h->ev_orth, h->stream)); HIPCK(h, hipStreamWaitEvent(h->side_stream, h->ev_orth, 0)); }
    return RSREC_OK;
}
int side_reduce_end(rsrec_t* h, SideReduce& S) { if (S.side) { HIPCK(h, hipEventRecord(h->ev_bred, h->side_stream)); S.pending = true; } return RSREC_OK; }
int side_reduce_wait(rsrec_t* h, SideReduce& S) { if (S.pending) { HIPCK(h, hipStreamWaitEvent(h->stream, h->ev_bred, 0)); S.pending = false; } return RSREC_OK; }

// Runs `enqueue` -- stream work only: kernels, memsets, cross-stream events -- as the handle's HIP graph: captured and instantiated when
// `key` (everything the nodes hold by value) differs from that of the graph the handle keeps, replayed otherwise.  The level loop of a
// small block-Lanczos batch is captured ONCE and replayed by every later call with the same lattice, seeds, depth and buffers (each SCF
// iteration of the reference: recur_b on the same <= 4 sites) -- 49 levels x 6-8 dependent launches otherwise cost more host time than
// device time (13 ms for one site of the 22^3 cell, two thirds of it launch latency).
template <class Enqueue>
int replay_level_loop(rsrec_t* h, const std::vector<uintptr_t>& key, Enqueue&& enqueue) {
    if (!h->graph_exec || key != h->graph_key) {
        if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
        h->graph_key.clear();
        s5_prepare(h);
        XFER(s4_prepare(h));
        HIPCK(h, hipStreamSynchronize(h->stream));
        HIPCK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed));
        h->capturing = true;
        const int rc = enqueue();
        h->capturing = false;
        hipGraph_t graph = nullptr;
        const hipError_t ec = hipStreamEndCapture(h->stream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (ec != hipSuccess || !graph) return fail(h, RSREC_ERR_DEVICE, "hipStreamEndCapture failed: %s", hipGetErrorString(ec));
        const hipError_t ei = hipGraphInstantiate(&h->graph_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ei != hipSuccess) { h->graph_exec = nullptr; return fail(h, RSREC_ERR_DEVICE, "hipGraphInstantiate failed: %s", hipGetErrorString(ei)); }
        h->graph_key = key;
    }
    HIPCK(h, hipGraphLaunch(h->graph_exec, h->stream));
    return RSREC_OK;
}

// Local-axis runs: A' = R^H A R, B'^2 = R^H B^2 R on the resident copy of chains c0 .. c0 + nb - 1, which is then what the caller gets back
// and what the stages on resident chains read -- one set of bits (get_terminf is a chain of bisections)
int rotate_resident_coef(rsrec_t* h, RecursionCall& RC, double2* dA, double2* dB, int c0, int nb, int lld) {
    hipEvent_t r0 = next_event(h);
    k_rotate_coef<<<dim3(2 * (lld - 1), nb), 256, 0, h->stream>>>(dA, dB, h->d_rot.as<double2>() + (size_t)c0 * BLK, lld);
    HIPCK(h, hipGetLastError());
    RC.rot_ev.emplace_back(r0, next_event(h));
    return RSREC_OK;
}
// End of a recursion: the status word and the timing; on success the chains' coefficients are the handle's resident ones (res_kind, see there)
int recursion_end(rsrec_t* h, const RecursionCall& RC, int res_kind, int lld, bool seeded) {
    hipEvent_t ev_end = next_event(h);
    const int rc = finish_status(h);
    finish_timing(h, RC.ev_begin, ev_end, RC.hop_ev);
    for (auto& pr : RC.rot_ev) h->t_rot_ms += ev_ms(pr.first, pr.second);
    if (rc) return rc;
    h->res_kind = res_kind; h->res_n = RC.nchains; h->res_lld = lld; h->res_seeded = seeded;
    return RSREC_OK;
}

// One implementation for both kernel sets: L = LayoutCM with the VALU kernels, LayoutRM with the MFMA SpMM.
// Work vectors.  Matrix-core set without hoh: vector 1 (pmn of the VALU set, h psi of the hoh passes) is not used by the u-scheme -- it is neither allocated
// nor cleared (32 GB and a 5 ms memset per call for 64 sites of the 10^5-atom cell).  Of vector 2, H psi, only the zero block kk is
// cleared: the SpMM writes every atom the passes behind it read, but those passes run padding entries of the lists as the zero block,
// which has to BE zero in every vector (left uncleared on recycled device memory, dying chains of the fuzz seeds survived:
// tests/test_gpu_breakdown.py).  46^3 x 64 sites: 2 387 -> 2 361-2 381 ms per step.
// u_{n+1} goes into a THIRD u vector instead of over u_{n-1} (option orth_oop, round 4): k_mfma_orth3 then reads three vectors and writes a
// fourth one -- 64 x 46^3: 25.7 -> 24.5 ms per saturated level (the in-place pass alternated 26.3 / 25.0 with the level's parity, the out-of-place
// one cycles 25.0 / 25.6 / 22.9 with the three arrangements of its buffers), the step 2 387 -> 2 361 ms, 22^3 387 -> 379 ms; bitwise the same results.
// The vector is number 1 without hoh (unused by the u-scheme otherwise) and number 4 with hoh (vector 1 holds h psi of the first pass).
template <class L, bool MFMA>
int run_block_lanczos(rsrec_t* h, int nchains, int nseed, const int32_t* seed_atoms, const double* seed_coef, int lld, double* a_b, double* b2_b,
                      const double* rot = nullptr /*local-axis runs: complex (18,18,nchains), the spin-frame rotation of every chain*/) {
    const int kk = h->kk;
    const bool hoh = h->hoh != 0;
    const int nsteps = lld - 1;
    if (rot && !MFMA) return fail(h, RSREC_ERR_ARG, "local-axis recursion needs the matrix-core kernel set (option kernels = 0 or 2)");
    RecursionCall RC = recursion_call(h, MFMA, nchains, nseed, nsteps, rot);
    const int ci = RC.ci, ntau = h->nmax + h->ntype;
    const size_t cstride = (size_t)lld * BLK, orth_lds = TILE_ATOMS * BLK * sizeof(double2);
    // the coefficients of ALL chains of the call stay on the device (resident input of rsrec_pack_diag / rsrec_block_ldos): reserved before
    // the batch is planned from the free memory
    drop_resident(h);
    HIPCK(h, h->d_coefA.reserve((size_t)nchains * lld * BLK * sizeof(double2)));
    HIPCK(h, h->d_coefB.reserve((size_t)nchains * lld * BLK * sizeof(double2)));
    if (rot) {                                          // the rotations of all chains, once per call (k_rotate_coef)
        HIPCK(h, h->d_rot.reserve((size_t)nchains * BLK * sizeof(double2)));
        XFER(xfer_h2d(h, h->d_rot.p, rot, (size_t)nchains * BLK * sizeof(double2)));
    }
    const bool oop = MFMA && h->opt_orth_oop != 0 && h->opt_orth3 != 2;
    const int nvec = MFMA ? (oop && hoh ? 5 : 4) : (hoh ? 3 : 2);
    const bool use_v1 = !MFMA || hoh || oop;
    // The A_n Gram in k_spmm5's epilogue: block Lanczos on the matrix-core set with k_spmm5, a Hermitian operator of one class, no hoh, no
    // per-chain stream heads, whole-group waves, and images enough for k_gram_groupsum in every launch of the post-hop passes.  A property of
    // the operator and the options, never of the launch; which (chain, level) passes then fold is s5_gram_folds on the chain's group count.
    const size_t gram_groups = ((size_t)kk + 7 * (size_t)(h->nmax + h->ntype) + 8 + GROUP - 1) / GROUP;      // no list is longer
    const bool gram_eligible = MFMA && ci && !hoh && !rot && h->ntype == 1 && h->nmax == 0 && h->ham_hermitian && h->opt_s5_split != 3 &&
                               RC.op->single_class(0) >= 0 && (h->opt_nblk <= 0 || 2 * h->opt_nblk >= S5_GRAM_MAXW) &&
                               s5_gram_folds((long)gram_groups, h->opt_s5_gram_min);
    const size_t gram_cstride = gram_eligible ? gram_groups * 2 * S5_GRAM_DOUBLES : 0;
    XFER(recursion_begin(h, RC, nvec, use_v1 ? -1 : 1, nseed, gram_cstride));
    const int B = RC.B, nblk = RC.nblk;
    HIPCK(h, h->d_frags.reserve((size_t)B * 3 * 27 * 64 * sizeof(double)));
    HIPCK(h, h->d_bmats.reserve((size_t)B * 2 * BLK * sizeof(double2)));
    const size_t gram_elems = (size_t)B * 256 * 1296;    // doubles: Gram partials of one kernel (<= 256 workgroups per chain)
    double *pmn = h->d_vec[1].as<double>(), *hpsi = h->d_vec[2].as<double>();
    double2* partial = h->d_partial.as<double2>();
    double *gpartial = h->d_partial.as<double>(), *bfrags = h->d_frags.as<double>();   // bfrags [chain][3][27 * 64]: the three right-multiply tables of k_mfma_orth3
    HIPCK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_orth<L>), hipFuncAttributeMaxDynamicSharedMemorySize, TILE_ATOMS * BLK * (int)sizeof(double2)));
    h->hop_fuses_a = MFMA ? 0 : 1;

    for (int c0 = 0; c0 < nchains; c0 += B) {
        const int nb = std::min(B, nchains - c0);
        double2* dA = h->d_coefA.as<double2>() + (size_t)c0 * cstride;       // this batch's slice of the resident coefficients
        double2* dB = h->d_coefB.as<double2>() + (size_t)c0 * cstride;
        RecursionBatch bt;
        XFER(recursion_batch(h, RC, seed_atoms, seed_coef, c0, nb, bt));
        const ChainView &CV = bt.CV, &CVp = bt.CVp;
        // what folds at a level: 0 no chain, 1 some chains (k_mfma_adot serves the others), 2 every chain (no k_mfma_adot launch)
        const rsrec_handle::RegionEntry* RE = h->cur_entry;
        auto fold_at = [&](int lv) -> int {
            if (!gram_eligible || !RE || lv < 0 || lv >= (int)RE->hop_max.size()) return 0;
            if (!s5_gram_folds(RE->hop_max[lv] / GROUP, h->opt_s5_gram_min)) return 0;
            return s5_gram_folds(RE->hop_min[lv] / GROUP, h->opt_s5_gram_min) ? 2 : 1;
        };
        for (int ll = 0; ll < nsteps; ++ll) { const int f = fold_at(ll + 1); h->n_gram_folded += f > 0; h->n_gram_all += f == 2; h->n_gram_levels += 1; }
        // everything from here to the coefficients' download is stream work only: small batches replay it as a HIP graph
        auto enqueue_levels = [&]() -> int {
            XFER(clear_vectors(h, RC, nb, MFMA && !hoh ? 2 : -1));
            HIPCK(h, hipMemsetAsync(dA, 0, (size_t)nb * cstride * sizeof(double2), h->stream));
            HIPCK(h, hipMemsetAsync(dB, 0, (size_t)nb * cstride * sizeof(double2), h->stream));
            if (MFMA) HIPCK(h, hipMemsetAsync(bfrags, 0, (size_t)nb * 3 * 27 * 64 * sizeof(double), h->stream));
            double *psi = h->d_vec[0].as<double>(), *t2 = h->d_vec[3].as<double>();   // (swapped every level)
            double* t3 = oop ? h->d_vec[hoh ? 4 : 1].as<double>() : nullptr;
            seed_chains(h, RC, nb, psi);
            k_set_identity<<<nb, 256, 0, h->stream>>>(dB, cstride);                                  // b2temp_b(:,:,1) = I  (:1837)
            if (MFMA) k_uscheme_init<<<nb, 256, 0, h->stream>>>(h->d_bmats.as<double2>(), bfrags, ci);
            const dim3 grid(nblk, nb);
            // u-scheme: H u_{n+1} does not need B_{n+1}, so the reduction of sum u_{n+1}^H u_{n+1} and its 18x18 eigen-solve (one
            // workgroup per chain, 80 us) leave the critical path: they run on the side stream while the main stream already applies H.
            // The main stream waits for them before k_reduce_a_u of the next level (first consumer of Binv_{n+1}).
            SideReduce SR{RC.side};
            double* gp_b = SR.side ? gpartial + gram_elems : gpartial;   // Gram partials of k_mfma_orth3: their own when the side stream reduces them
            for (int ll = 0; ll < nsteps; ++ll) {
                const int lv_final = hoh ? 2 * ll + 2 : ll + 1;
                if (MFMA) {
                    // matrix-core kernel set, un-normalised vectors (kernels_uscheme.hpp): psi = u_n, t2 = u_{n-1}; u_{n+1} overwrites u_{n-1}
                    // (with hoh, h psi of the first pass goes into the pmn buffer, free in the u-scheme)
                    const int folds = fold_at(lv_final);
                    const GramFold GF{folds ? CV.cum : nullptr, RC.nlev, h->opt_s5_gram_min};
                    XFER(apply_h(h, RC, bt, ll + 1, psi, hpsi, pmn, bt.la_extra, ntau, S5Epilogue(),
                                 folds ? S5Gram{h->d_gram.as<double>(), gram_cstride, h->opt_s5_gram_min} : S5Gram()));
                    const dim3 gl = level_grid(h, bt.grid_mf, lv_final);
                    if (folds < 2) k_mfma_adot<<<gl, MF_WAVES * 64, 0, h->stream>>>(CVp, lv_final, kk, psi, hpsi, gpartial, GF);
                    if (folds) k_gram_groupsum<<<gl, 384, 0, h->stream>>>(GF, lv_final, h->d_gram.as<double>(), gram_cstride, gpartial);
                    int n2 = gl.x; const double* p2 = presum(h, gpartial, nb, n2, 1296);
                    XFER(side_reduce_wait(h, SR));
                    k_reduce_a_u<<<nb, 1024, 0, h->stream>>>(p2, n2, dA + (size_t)ll * BLK, cstride, h->d_bmats.as<double2>(), bfrags, ci);
                    if (h->opt_orth3 == 2) k_mfma_orth3w<<<gl, MF_WAVES * 64, 0, h->stream>>>(CVp, lv_final, kk, hpsi, psi, t2, bfrags, gp_b);
                    else k_mfma_orth3<<<gl, MF_WAVES * 64, 0, h->stream>>>(CVp, lv_final, kk, hpsi, psi, t2, bfrags, gp_b, t3);
                    hipStream_t st; XFER(side_reduce_begin(h, SR, st));
                    n2 = gl.x; p2 = presum(h, gp_b, nb, n2, 1296, st, SR.side ? 1 : 0);
                    k_reduce_b_u<<<nb, 1024, 0, st>>>(p2, n2, dB + (size_t)(ll + 1) * BLK, cstride, h->d_bmats.as<double2>(), bfrags, h->d_status.as<int>(), ci);
                    XFER(side_reduce_end(h, SR));
                    if (oop) { double* f = t2; t2 = psi; psi = t3; t3 = f; }      // u_{n+1} is in t3; the vector of u_{n-1} is free
                    else std::swap(psi, t2);
                    continue;
                }
                // FP64 VALU kernel set: the reference's literal order on the reference's layout
                XFER((valu_apply_h<AM_LANCZOS, AM_HOH_LANCZOS>(h, RC, bt, ll + 1, psi, psi, pmn, hpsi)));
                k_reduce_a<<<nb, 1024, 0, h->stream>>>(partial, nblk, dA + (size_t)ll * BLK, cstride);
                k_orth<L><<<grid, NTHREADS, orth_lds, h->stream>>>(CV, lv_final, psi, pmn, (const double*)nullptr, dA + (size_t)ll * BLK, cstride, partial);
                k_reduce_b_eig<<<nb, 1024, 0, h->stream>>>(partial, nblk, dB + (size_t)(ll + 1) * BLK, cstride, h->d_bmats.as<double2>(), h->d_status.as<int>());
                k_update<L><<<grid, NTHREADS, 0, h->stream>>>(CV, lv_final, psi, pmn, h->d_bmats.as<double2>());
            }
            HIPCK(h, hipGetLastError());
            return side_reduce_wait(h, SR);
        };
        const bool use_graph = MFMA && nchains <= B && ((h->opt_graph == 1 && nchains <= 8) || h->opt_graph >= 2) && getenv("RSREC_NO_GRAPH") == nullptr;
        if (!use_graph) XFER(enqueue_levels());
        else {
            if (ci) HIPCK(h, h->d_s5queue.reserve((size_t)nb * 16 * sizeof(int)));
            const Spmm5Operator& OP = *RC.op;
            // what the nodes hold BY VALUE: every pointer and dimension a kernel argument is made of
            std::vector<uintptr_t> key = {(uintptr_t)1 /*block Lanczos*/, (uintptr_t)nb, (uintptr_t)lld, (uintptr_t)nseed, (uintptr_t)hoh, (uintptr_t)ci, (uintptr_t)(rot != nullptr), (uintptr_t)kk,
                                          (uintptr_t)bt.CV.order, (uintptr_t)bt.CV.cum, (uintptr_t)bt.ostride, (uintptr_t)OP.d_frag, (uintptr_t)OP.d_meta, (uintptr_t)OP.ntr,
                                          (uintptr_t)h->s4_op.frag_set(0), (uintptr_t)h->s4_op.meta_set(0), (uintptr_t)h->d_nbr.p, (uintptr_t)h->d_nbr5.p, (uintptr_t)h->d_iz.p,
                                          (uintptr_t)h->d_partial.p, (uintptr_t)h->d_partial2.p, (uintptr_t)h->d_frags.p, (uintptr_t)dA, (uintptr_t)dB, (uintptr_t)h->d_bmats.p,
                                          (uintptr_t)h->d_status.p, (uintptr_t)h->d_seed.p, (uintptr_t)h->d_seedcoef.p, (uintptr_t)h->d_la_extra.p, (uintptr_t)h->d_s5queue.p,
                                          (uintptr_t)h->cur_entry->serial, (uintptr_t)h->p2_slot, (uintptr_t)OP.single_class(0), (uintptr_t)OP.spin_mixing,
                                          (uintptr_t)h->lattice_epoch, (uintptr_t)OP.sched_epoch, (uintptr_t)h->nslots, (uintptr_t)h->nmax, (uintptr_t)h->ntype, (uintptr_t)h->hslots,
                                          (uintptr_t)B, (uintptr_t)h->n_cu, (uintptr_t)h->d_gram.p, (uintptr_t)gram_eligible};
            for (int v = 0; v < nvec; ++v) key.push_back((uintptr_t)h->d_vec[v].p);
            // ... and every option: launch shapes and kernel choices follow them (all but `graph`, which only decides whether this path is taken)
            for (const OptionEntry& o : OPTIONS)
                if (o.member != &rsrec_handle::opt_graph) key.push_back((uintptr_t)(h->*o.member));
            XFER(replay_level_loop(h, key, enqueue_levels));
            h->n_hop_launch += (double)nsteps * (hoh ? 2 : 1);
        }
        if (rot && lld > 1) XFER(rotate_resident_coef(h, RC, dA, dB, c0, nb, lld));
        XFER(xfer_d2h(h, a_b + (size_t)c0 * cstride * 2, dA, (size_t)nb * cstride * sizeof(double2)));
        XFER(xfer_d2h(h, b2_b + (size_t)c0 * cstride * 2, dB, (size_t)nb * cstride * sizeof(double2)));
        HIPCK(h, hipStreamSynchronize(h->stream));
    }
    if (MFMA && h->n_gram_levels > 0 && h->n_gram_all == h->n_gram_levels) h->hop_fuses_a = 1;   // every H|psi> launch also formed the A_n Gram
    return recursion_end(h, RC, 1, lld, seed_coef != nullptr);
}

}  // namespace

extern "C" int rsrec_block_lanczos_seeded(rsrec_t* h, int nchains, int nseed, const int32_t* seed_atoms, const double* seed_coef, int lld,
                                          double* a_b, double* b2_b) {
    int rc = check_ready(h, "rsrec_block_lanczos");
    if (rc) return rc;
    if (nchains < 0 || nseed < 1 || lld < 1 || !a_b || !b2_b || (nchains > 0 && !seed_atoms)) return fail(h, RSREC_ERR_ARG, "rsrec_block_lanczos: bad argument");
    XFER(check_seeds(h, "rsrec_block_lanczos", seed_atoms, (size_t)nchains * nseed, 1));
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    if (nchains == 0) return RSREC_OK;
    if (matrix_core_set(h)) return run_block_lanczos<LayoutRM, true>(h, nchains, nseed, seed_atoms, seed_coef, lld, a_b, b2_b);
    return run_block_lanczos<LayoutCM, false>(h, nchains, nseed, seed_atoms, seed_coef, lld, a_b, b2_b);
}

extern "C" int rsrec_block_lanczos(rsrec_t* h, int nsites, const int32_t* seed_atoms, int lld, double* a_b, double* b2_b) {
    return rsrec_block_lanczos_seeded(h, nsites, 1, seed_atoms, nullptr, lld, a_b, b2_b);
}

namespace {

// Operator tables of a local-axis run: the blocks as set (GLOBAL spin frame), on-site slot WITHOUT l.s; the l.s term (with e_nu for
// hoh) enters through the extra on-site slot whose fragments come per chain.  The placeholder only makes the slot appear in the
// schedule with both spin parts.
int build_local_axis_operator(rsrec_t* h) {
    if (h->s5_la_ok) return RSREC_OK;
    const int ntau = h->nmax + h->ntype, nfs = h->nslots + 1, nset = h->hoh ? 2 : 1;
    const size_t B = 2 * (size_t)BLK;
    std::vector<const double*> blk((size_t)nset * ntau * nfs, nullptr);
    std::vector<double> dense(B, 1.0), neg((size_t)ntau * h->nslots * B, 0.0);
    for (int tau = 0; tau < ntau; ++tau) {
        for (int s = 0; s < h->nslots; ++s) {
            const double* src = tau < h->nmax ? h->host_hall.data() + B * (s + (size_t)h->hslots * tau) : h->host_ee.data() + B * (s + (size_t)h->hslots * (tau - h->nmax));
            blk[((size_t)0 * ntau + tau) * nfs + s] = src;
            if (nset > 1) {
                const double* so = tau < h->nmax ? h->host_hallo.data() + B * (s + (size_t)h->hslots * tau) : h->host_eeo.data() + B * (s + (size_t)h->hslots * (tau - h->nmax));
                double* d = neg.data() + B * (s + (size_t)h->nslots * tau);
                for (size_t e = 0; e < B; ++e) d[e] = -so[e];
                if (s == 0) for (int q = 0; q < NB; ++q) d[2 * (q + NB * q)] += 1.0;
                blk[((size_t)1 * ntau + tau) * nfs + s] = d;
            }
        }
        blk[((size_t)(nset - 1) * ntau + tau) * nfs + h->nslots] = dense.data();
    }
    const char* msg = h->s5_la.build_custom(h->nslots, ntau, nset, blk);
    if (msg) return fail(h, RSREC_ERR_DEVICE, "rsrec_block_lanczos_local_axis: %s", msg);
    h->s5_la_ok = 1;
    return RSREC_OK;
}

}  // namespace

// recur_b with hamiltonian%local_axis = T (recursion.f90:1830-1832), all sites in one batched call.  The reference rotates every
// block into the spin frame of site i's moment before that site's chain, H'_i = R_i^H H R_i blockwise -- except the on-site l.s term,
// which rotate_to_local_axis (hamiltonian.f90:2442-2465) leaves alone.  With phi = R_i psi (blocks multiplied from the left) the
// chain of H'_i from the seed 1 is the chain of  H''_i = H + onsite(R_i l.s R_i^H - l.s)  from the seed R_i, i.e. from the seed 1
// followed by a right-multiplication with the unitary R_i:   A'_n = R_i^H A''_n R_i,  B'^2_n = R_i^H B''^2_n R_i.
// So every chain runs on the SAME global-frame blocks and differs only in its on-site term (per-chain extra slot of k_spmm5); the
// 18x18 coefficients are conjugated where they lie on the device (k_rotate_coef) before they are downloaded: the returned arrays and the
// resident chains are one set of bits, in each site's local frame.  The continued fraction, zsqr, get_terminf and the epilogues are covariant
// under the transform, so rsrec_block_ldos / _spectra / rsrec_contour_occupation / rsrec_pack_diag follow as after rsrec_block_lanczos.
// Checked against the compiled reference on four sites with four moment directions.
extern "C" int rsrec_block_lanczos_local_axis(rsrec_t* h, int nsites, const int32_t* seed_atoms, const double* rot, int lld, double* a_b, double* b2_b) {
    int rc = check_ready(h, "rsrec_block_lanczos_local_axis");
    if (rc) return rc;
    if (nsites < 0 || lld < 1 || !a_b || !b2_b || (nsites > 0 && (!seed_atoms || !rot))) return fail(h, RSREC_ERR_ARG, "rsrec_block_lanczos_local_axis: bad argument");
    XFER(check_seeds(h, "rsrec_block_lanczos_local_axis", seed_atoms, (size_t)nsites, 1));
    if (!h->s5_built) return fail(h, RSREC_ERR_ARG, "rsrec_block_lanczos_local_axis: lattice has too many neighbour slots for the SpMM kernel");
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    if (nsites == 0) return RSREC_OK;
    rc = build_local_axis_operator(h); if (rc) return rc;
    // the chains stay resident in each site's frame (res_kind = 1): the stages on resident chains take them as they take rsrec_block_lanczos'
    return run_block_lanczos<LayoutRM, true>(h, nsites, 1, seed_atoms, nullptr, lld, a_b, b2_b, rot);
}

namespace {

// true if p is device memory of this process (torch / hipMalloc allocations): outputs may then stay on the GPU.
// A Python process that imports torch holds TWO HIP runtimes (torch bundles its own libamdhip64; this library links the system one)
// on top of ONE shared ROCr/HSA runtime and one GPU address space: a tensor's address is valid in our kernels, but our HIP runtime
// has never heard of it.  So the question is put to ROCr (hsa_amd_pointer_info), which knows every allocation of the process.
bool is_device_ptr(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) == hipSuccess) return at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    hsa_amd_pointer_info_t info;
    memset(&info, 0, sizeof info);
    info.size = sizeof info;
    if (hsa_amd_pointer_info(const_cast<void*>(p), &info, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS) return false;
    if (info.type != HSA_EXT_POINTER_TYPE_HSA) return false;                          // unknown = plain pageable host memory
    hsa_device_type_t dt = HSA_DEVICE_TYPE_CPU;
    if (hsa_agent_get_info(info.agentOwner, HSA_AGENT_INFO_DEVICE, &dt) != HSA_STATUS_SUCCESS) return false;
    return dt == HSA_DEVICE_TYPE_GPU;
}

// a(ll, l, site) = Re a_b(l, l, ll, site), b2 likewise (recursion.f90:1850-1851), written into zero-padded images over all sites
__global__ void k_pack_diag(const double2* __restrict__ A, const double2* __restrict__ B, int lld, int n, int off, int ntot,
                            double* __restrict__ a_img, double* __restrict__ b_img) {
    const size_t total = (size_t)lld * NB * ntot;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int ll = (int)(e % lld), l = (int)((e / lld) % NB), s = (int)(e / ((size_t)lld * NB)) - off;
        double a = 0.0, b = 0.0;
        if (s >= 0 && s < n) {
            const size_t q = ((size_t)s * lld + ll) * BLK + (size_t)l * (NB + 1);
            a = A[q].x; b = B[q].x;
        }
        a_img[e] = a; b_img[e] = b;
    }
}

}  // namespace

// The per-site result the ranks exchange after the recursion, packed on the device: bands.f90:271-274 gathers per-site arrays with
// MPI_ALLREDUCE(MPI_SUM) on zero-padded images; this writes this rank's part of such an image (every other site zero).
extern "C" int rsrec_pack_diag(rsrec_t* h, int site_offset, int nsites_total, double* a_img, double* b2_img) {
    if (!h || !a_img || !b2_img || site_offset < 0) return fail(h, RSREC_ERR_ARG, "rsrec_pack_diag: bad argument");
    if (h->res_kind != 1) return fail(h, RSREC_ERR_ARG, "rsrec_pack_diag: no block-Lanczos coefficients resident (call rsrec_block_lanczos first)");
    if (site_offset + h->res_n > nsites_total) return fail(h, RSREC_ERR_ARG, "rsrec_pack_diag: sites %d..%d outside 1..%d", site_offset + 1, site_offset + h->res_n, nsites_total);
    HIPCK(h, hipSetDevice(h->device));
    const size_t n = (size_t)h->res_lld * NB * nsites_total;
    const bool dev = is_device_ptr(a_img) && is_device_ptr(b2_img);
    double *da = a_img, *db = b2_img;
    if (!dev) { HIPCK(h, h->d_scal.reserve(2 * n * sizeof(double))); da = h->d_scal.as<double>(); db = da + n; }
    const int blocks = (int)std::min<size_t>(1024, (n + 255) / 256);
    k_pack_diag<<<blocks, 256, 0, h->stream>>>(h->d_coefA.as<double2>(), h->d_coefB.as<double2>(), h->res_lld, h->res_n, site_offset, nsites_total, da, db);
    HIPCK(h, hipGetLastError());
    if (!dev) { XFER(xfer_d2h(h, a_img, da, n * sizeof(double))); XFER(xfer_d2h(h, b2_img, db, n * sizeof(double))); }
    HIPCK(h, hipStreamSynchronize(h->stream));
    return RSREC_OK;
}

namespace {

// mu_n(18,18,nmom,site) of this rank's sites inside a zero image over all sites
__global__ void k_pack_moments(const double2* __restrict__ mu, size_t per_site, int n, int off, int ntot, double2* __restrict__ img) {
    const size_t total = per_site * (size_t)ntot;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int s = (int)(e / per_site) - off;
        img[e] = (s >= 0 && s < n) ? mu[(size_t)s * per_site + e % per_site] : make_double2(0.0, 0.0);
    }
}

}  // namespace

// The Chebyshev counterpart of rsrec_pack_diag: the moments mu_n(18,18,2 lld + 2,site) of the last rsrec_chebyshev call, as they lie on
// the device, written into a zero-padded image over all sites (the buffer a sum all-reduce turns into the all-gather the reference's
// commented-out MPI_Allgather of recursion.f90:1790-1793 describes).  mu_img: device or host memory, complex (18,18,2 lld + 2,nsites_total).
extern "C" int rsrec_pack_moments(rsrec_t* h, int site_offset, int nsites_total, double* mu_img) {
    if (!h || !mu_img || site_offset < 0) return fail(h, RSREC_ERR_ARG, "rsrec_pack_moments: bad argument");
    if (h->res_kind != 2) return fail(h, RSREC_ERR_ARG, "rsrec_pack_moments: no Chebyshev moments resident (call rsrec_chebyshev first)");
    if (site_offset + h->res_n > nsites_total) return fail(h, RSREC_ERR_ARG, "rsrec_pack_moments: sites %d..%d outside 1..%d", site_offset + 1, site_offset + h->res_n, nsites_total);
    HIPCK(h, hipSetDevice(h->device));
    const size_t per_site = (size_t)(2 * h->res_lld + 2) * BLK, n = per_site * nsites_total;
    const bool dev = is_device_ptr(mu_img);
    double2* out = reinterpret_cast<double2*>(mu_img);
    if (!dev) { HIPCK(h, h->d_scal.reserve(n * sizeof(double2))); out = h->d_scal.as<double2>(); }
    k_pack_moments<<<(int)std::min<size_t>(2048, (n + 255) / 256), 256, 0, h->stream>>>(h->d_mu.as<double2>(), per_site, h->res_n, site_offset, nsites_total, out);
    HIPCK(h, hipGetLastError());
    if (!dev) XFER(xfer_d2h(h, mu_img, out, n * sizeof(double2)));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return RSREC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Library-level communicator.  The reference's only exchange on this path is MPI_ALLREDUCE(MPI_IN_PLACE, ..., MPI_SUM) on zero-padded
// per-site arrays (bands.f90:271-274; mpi.f90:32-58 gives every rank whole sites).  On a node of MI355X this is one RCCL all-reduce
// over xGMI on a device image; RCCL is bound with dlopen when a communicator is asked for -- the recursion itself does not depend on
// it -- so a Fortran (or any) host needs neither MPI nor torch for it: the 128-byte id travels by whatever the host has (MPI_Bcast, a
// file on a shared directory: rsrec_comm_init_file).
namespace {

struct NcclId { char internal[RSREC_COMM_ID_BYTES]; };
struct RcclApi {
    void* lib = nullptr;
    int (*get_unique_id)(NcclId*) = nullptr;
    int (*comm_init_rank)(void**, int, NcclId, int) = nullptr;
    int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*comm_destroy)(void*) = nullptr;
    const char* (*get_error_string)(int) = nullptr;
};
RcclApi g_rccl;

const char* rccl_ready() {
    if (g_rccl.lib) return nullptr;
    void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) return "RCCL (librccl.so) not found";
    g_rccl.get_unique_id = reinterpret_cast<decltype(g_rccl.get_unique_id)>(dlsym(lib, "ncclGetUniqueId"));
    g_rccl.comm_init_rank = reinterpret_cast<decltype(g_rccl.comm_init_rank)>(dlsym(lib, "ncclCommInitRank"));
    g_rccl.all_reduce = reinterpret_cast<decltype(g_rccl.all_reduce)>(dlsym(lib, "ncclAllReduce"));
    g_rccl.comm_destroy = reinterpret_cast<decltype(g_rccl.comm_destroy)>(dlsym(lib, "ncclCommDestroy"));
    g_rccl.get_error_string = reinterpret_cast<decltype(g_rccl.get_error_string)>(dlsym(lib, "ncclGetErrorString"));
    if (!g_rccl.get_unique_id || !g_rccl.comm_init_rank || !g_rccl.all_reduce || !g_rccl.comm_destroy) return "RCCL symbols missing";
    g_rccl.lib = lib;
    return nullptr;
}
const char* rccl_err(int rc) { return g_rccl.get_error_string ? g_rccl.get_error_string(rc) : "RCCL error"; }

}  // namespace

// id: RSREC_COMM_ID_BYTES bytes; created by ONE rank and given to all (ncclGetUniqueId).
extern "C" int rsrec_comm_unique_id(char* id) {
    if (!id) return RSREC_ERR_ARG;
    if (rccl_ready()) return RSREC_ERR_DEVICE;
    NcclId u;
    if (g_rccl.get_unique_id(&u) != 0) return RSREC_ERR_DEVICE;
    memcpy(id, u.internal, RSREC_COMM_ID_BYTES);
    return RSREC_OK;
}

extern "C" int rsrec_comm_destroy(rsrec_t* h) {
    if (!h) return RSREC_ERR_ARG;
    if (h->comm) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        (void)g_rccl.comm_destroy(h->comm);
        h->comm = nullptr;
    }
    h->comm_rank = 0; h->comm_nranks = 1;
    return RSREC_OK;
}

// Collective over all ranks: every rank calls it with the same id and its own rank; the handle's device is the rank's GPU.
extern "C" int rsrec_comm_init(rsrec_t* h, int rank, int nranks, const char* id) {
    if (!h || !id || nranks < 1 || rank < 0 || rank >= nranks) return fail(h, RSREC_ERR_ARG, "rsrec_comm_init: bad argument");
    if (const char* msg = rccl_ready()) return fail(h, RSREC_ERR_DEVICE, "rsrec_comm_init: %s", msg);
    (void)rsrec_comm_destroy(h);
    HIPCK(h, hipSetDevice(h->device));
    NcclId u;
    memcpy(u.internal, id, RSREC_COMM_ID_BYTES);
    const int rc = g_rccl.comm_init_rank(&h->comm, nranks, u, rank);
    if (rc != 0) { h->comm = nullptr; return fail(h, RSREC_ERR_DEVICE, "ncclCommInitRank failed: %s", rccl_err(rc)); }
    h->comm_rank = rank; h->comm_nranks = nranks;
    return RSREC_OK;
}

// The same with the id exchanged through a file (hosts without MPI): rank 0 creates the id and publishes it at `path` (written to a
// temporary name, then renamed: readers never see a partial file); the other ranks wait for it up to `timeout_s` seconds.  `path` must
// be fresh for every communicator (rank 0 replaces an existing file before the others may read a stale one only if they start later:
// use a per-job name).
extern "C" int rsrec_comm_init_file(rsrec_t* h, int rank, int nranks, const char* path, double timeout_s) {
    if (!h || !path || nranks < 1 || rank < 0 || rank >= nranks) return fail(h, RSREC_ERR_ARG, "rsrec_comm_init_file: bad argument");
    char id[RSREC_COMM_ID_BYTES];
    if (rank == 0) {
        if (rsrec_comm_unique_id(id) != RSREC_OK) return fail(h, RSREC_ERR_DEVICE, "rsrec_comm_init_file: ncclGetUniqueId failed");
        const std::string tmp = std::string(path) + ".tmp";
        FILE* f = fopen(tmp.c_str(), "wb");
        if (!f || fwrite(id, 1, sizeof id, f) != sizeof id) { if (f) fclose(f); return fail(h, RSREC_ERR_ARG, "rsrec_comm_init_file: cannot write %s", tmp.c_str()); }
        fclose(f);
        if (rename(tmp.c_str(), path) != 0) return fail(h, RSREC_ERR_ARG, "rsrec_comm_init_file: cannot publish %s", path);
    } else {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            FILE* f = fopen(path, "rb");
            if (f) {
                const size_t got = fread(id, 1, sizeof id, f);
                fclose(f);
                if (got == sizeof id) break;
            }
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
                return fail(h, RSREC_ERR_DEVICE, "rsrec_comm_init_file: no id at %s after %.0f s", path, timeout_s);
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
        }
    }
    return rsrec_comm_init(h, rank, nranks, id);
}

// In-place sum over the ranks of n doubles (the reference's MPI_ALLREDUCE(MPI_IN_PLACE, buf, n, MPI_DOUBLE_PRECISION, MPI_SUM, ...),
// bands.f90:271-274).  buf: DEVICE memory (the images rsrec_pack_diag / rsrec_pack_moments / rsrec_block_ldos wrote: reduced where they
// lie, on the engine's stream) or host memory (staged through the device).  Returns when the result is in buf.  Without a communicator
// (or with one rank) it is the identity, like the reference built without MPI.
extern "C" int rsrec_allreduce_sum(rsrec_t* h, double* buf, size_t n) {
    if (!h || (!buf && n > 0)) return fail(h, RSREC_ERR_ARG, "rsrec_allreduce_sum: bad argument");
    if (n == 0) return RSREC_OK;
    HIPCK(h, hipSetDevice(h->device));
    if (!h->comm) { HIPCK(h, hipStreamSynchronize(h->stream)); return RSREC_OK; }
    const bool dev = is_device_ptr(buf);
    double* d = buf;
    if (!dev) {
        HIPCK(h, h->d_comm.reserve(n * sizeof(double)));
        d = h->d_comm.as<double>();
        XFER(xfer_h2d(h, d, buf, n * sizeof(double)));
    }
    const int rc = g_rccl.all_reduce(d, d, n, 8 /*ncclDouble*/, 0 /*ncclSum*/, h->comm, h->stream);
    if (rc != 0) return fail(h, RSREC_ERR_DEVICE, "ncclAllReduce failed: %s", rccl_err(rc));
    if (!dev) XFER(xfer_d2h(h, buf, d, n * sizeof(double)));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return RSREC_OK;
}

extern "C" int rsrec_comm_size(rsrec_t* h, int* rank, int* nranks) {
    if (!h) return RSREC_ERR_ARG;
    if (rank) *rank = h->comm_rank;
    if (nranks) *nranks = h->comm ? h->comm_nranks : 1;
    return RSREC_OK;
}

extern "C" int rsrec_zsqr(rsrec_t* h, int nmat, double* b2_b) {
    if (!h || nmat < 0 || (nmat > 0 && !b2_b)) return fail(h, RSREC_ERR_ARG, "rsrec_zsqr: bad argument");
    if (nmat == 0) return RSREC_OK;
    HIPCK(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)nmat * BLK * sizeof(double2);
    HIPCK(h, h->d_zsqr.reserve(bytes));              // (not d_mu: the Chebyshev moments of the last call stay resident there)
    HIPCK(h, h->d_status.reserve(64));
    HIPCK(h, hipMemsetAsync(h->d_status.p, 0, 64, h->stream));
    XFER(xfer_h2d(h, h->d_zsqr.p, b2_b, bytes));
    k_zsqr<<<nmat, 256, 0, h->stream>>>(h->d_zsqr.as<double2>(), h->d_status.as<int>());
    HIPCK(h, hipGetLastError());
    XFER(xfer_d2h(h, b2_b, h->d_zsqr.p, bytes));
    return finish_status(h);
}

namespace {

// The Green stage produces far more than it consumes (13 MB of g0 per site for 2510 energies): the sites are cut into chunks,
// chunk c + 1 is computed on h->stream while chunk c leaves the device on h->copy_stream (two output buffers).  The caller's
// array is pageable, so the copy blocks the host -- after the next kernel has been queued.
// launch(s0, ns, out): queue the kernel for sites s0 .. s0 + ns - 1 of the call, writing ns * gbytes bytes at `out`.
template <class Launch>
int green_pipeline(rsrec_t* h, int nsites, size_t gbytes, double* g0, Launch launch) {
    if (!h->copy_stream) HIPCK(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    for (hipEvent_t& e : h->ev_green)
        if (!e) HIPCK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const size_t cap = ((size_t)1 << 29) / gbytes;                                  // <= 2 x 512 MiB of g0 on the device
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(cap, ((size_t)nsites + 7) / 8));
    HIPCK(h, h->d_green_out.reserve(2 * (size_t)chunk * gbytes));
    char* out[2] = {static_cast<char*>(h->d_green_out.p), static_cast<char*>(h->d_green_out.p) + (size_t)chunk * gbytes};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans;
    auto drain = [&](int s0, int ns, int b) -> int {
        HIPCK(h, hipStreamWaitEvent(h->copy_stream, h->ev_green[b], 0));
        HIPCK(h, hipMemcpyAsync(reinterpret_cast<char*>(g0) + (size_t)s0 * gbytes, out[b], (size_t)ns * gbytes, hipMemcpyDeviceToHost, h->copy_stream));
        HIPCK(h, hipStreamSynchronize(h->copy_stream));
        return RSREC_OK;
    };
    int prev_s0 = -1, prev_ns = 0, c = 0;
    for (int s0 = 0; s0 < nsites; s0 += chunk, ++c) {
        const int ns = std::min(chunk, nsites - s0);
        hipEvent_t k0 = next_event(h);
        launch(s0, ns, out[c & 1]);
        hipEvent_t k1 = next_event(h);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipEventRecord(h->ev_green[c & 1], h->stream));
        spans.emplace_back(k0, k1);
        if (prev_s0 >= 0) XFER(drain(prev_s0, prev_ns, (c - 1) & 1));               // buffer (c - 1) & 1 is free again before kernel c + 1 is queued
        prev_s0 = s0; prev_ns = ns;
    }
    if (prev_s0 >= 0) XFER(drain(prev_s0, prev_ns, (c - 1) & 1));
    HIPCK(h, hipStreamSynchronize(h->stream));
    for (auto& sp : spans) h->t_hop_ms += ev_ms(sp.first, sp.second);              // "hop_ms": the Green kernels themselves; total_ms includes the transfers
    return RSREC_OK;
}

}  // namespace

// green%block_green / bgreen (green.f90:588-621, :1191-1339): g0(:,:,:,site) from the block coefficients of every site.
extern "C" int rsrec_block_green(rsrec_t* h, int nsites, int lld, int nen, const double* ene, double eta_re, double eta_im, int sym_term,
                                 const double* a_inf, const double* b_inf, const double* a_b, const double* b_sqrt, double* g0) {
    if (!h) return RSREC_ERR_ARG;
    if (nsites < 0 || lld < 1 || nen < 0 || (nsites > 0 && nen > 0 && (!ene || !a_inf || !b_inf || !a_b || !b_sqrt || !g0)))
        return fail(h, RSREC_ERR_ARG, "rsrec_block_green: bad argument");
    if (nsites == 0 || nen == 0) return RSREC_OK;
    HIPCK(h, hipSetDevice(h->device));
    const size_t cbytes = (size_t)lld * BLK * sizeof(double2);       // coefficients of one site (each of a_b, b_sqrt)
    const size_t tbytes = (size_t)BLK * sizeof(double);              // terminator of one site (each of a_inf, b_inf)
    const size_t gbytes = (size_t)nen * BLK * sizeof(double2);       // g0 of one site
    const size_t in_site = 2 * cbytes + 2 * tbytes;
    const int super = (int)std::max<size_t>(1, std::min<size_t>((size_t)nsites, ((size_t)4 << 30) / in_site));   // <= 4 GiB of coefficients resident
    release_kubo_buffers(h, true, true);
    HIPCK(h, h->d_green_in.reserve((size_t)super * in_site + (size_t)nen * sizeof(double)));
    char* base = static_cast<char*>(h->d_green_in.p);
    double* d_ene = reinterpret_cast<double*>(base);
    double2* d_ab = reinterpret_cast<double2*>(base + (size_t)nen * sizeof(double));
    double2* d_bs = reinterpret_cast<double2*>(reinterpret_cast<char*>(d_ab) + (size_t)super * cbytes);
    double* d_ai = reinterpret_cast<double*>(reinterpret_cast<char*>(d_bs) + (size_t)super * cbytes);
    double* d_bi = reinterpret_cast<double*>(reinterpret_cast<char*>(d_ai) + (size_t)super * tbytes);
    XFER(xfer_h2d(h, d_ene, ene, (size_t)nen * sizeof(double)));
    reset_timing(h);
    hipEvent_t ev0 = next_event(h);
    for (int u0 = 0; u0 < nsites; u0 += super) {
        const int nu = std::min(super, nsites - u0);
        XFER(xfer_h2d(h, d_ab, a_b + (size_t)u0 * lld * BLK * 2, (size_t)nu * cbytes));
        XFER(xfer_h2d(h, d_bs, b_sqrt + (size_t)u0 * lld * BLK * 2, (size_t)nu * cbytes));
        XFER(xfer_h2d(h, d_ai, a_inf + (size_t)u0 * BLK, (size_t)nu * tbytes));
        XFER(xfer_h2d(h, d_bi, b_inf + (size_t)u0 * BLK, (size_t)nu * tbytes));
        XFER(green_pipeline(h, nu, gbytes, g0 + (size_t)u0 * nen * BLK * 2, [&](int s0, int ns, char* out) {
            const dim3 grid((nen + GREEN_WAVES - 1) / GREEN_WAVES, ns);
            k_block_green<false><<<grid, GREEN_WAVES * 64, 0, h->stream>>>(lld, nen, d_ene, eta_re, eta_im, sym_term, d_ai + (size_t)s0 * BLK, d_bi + (size_t)s0 * BLK,
                                                                    d_ab + (size_t)s0 * lld * BLK, d_bs + (size_t)s0 * lld * BLK, reinterpret_cast<double2*>(out));
        }));
    }
    hipEvent_t ev1 = next_event(h);
    HIPCK(h, hipStreamSynchronize(h->stream));
    h->t_total_ms = ev_ms(ev0, ev1);
    return RSREC_OK;
}

namespace {

// Dynamic LDS for `kernel` beyond what `granted` records for it on this handle (the opt-in is per device: see s5_lds_limit)
int lds_opt_in(rsrec_t* h, const void* kernel, size_t bytes, size_t& granted) {
    if (bytes <= granted) return RSREC_OK;
    HIPCK(h, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    granted = bytes;
    return RSREC_OK;
}

// get_terminf for n sites on the device: a_inf, b_inf [site][324], optional means
int launch_terminator(rsrec_t* h, int n, int lld, const double2* d_ab, const double2* d_bs, double* d_ainf, double* d_binf) {
    if (lld < 2) return fail(h, RSREC_ERR_ARG, "terminator needs lld >= 2");
    // one LDS column of 2 * lld doubles per thread
    int T = 64;
    while (T > 8 && (size_t)2 * lld * T * sizeof(double) > (size_t)128 * 1024) T >>= 1;
    const size_t lds = (size_t)2 * lld * T * sizeof(double);
    if (lds > (size_t)150 * 1024) return fail(h, RSREC_ERR_ARG, "terminator: lld = %d too deep for the LDS staging", lld);
    XFER(lds_opt_in(h, reinterpret_cast<const void*>(k_terminator), lds, h->term_lds));
    k_terminator<<<dim3((BLK + T - 1) / T, n), T, lds, h->stream>>>(lld, d_ab, d_bs, d_ainf, d_binf);
    HIPCK(h, hipGetLastError());
    return RSREC_OK;
}

// The block prologue on the resident chains c0 .. c0 + nc - 1, for every stage that reads them (SiteStage, PairCall).  b2_b of the recursion
// stays B^2 -- the caller may still fetch it, and the next stage starts from it again -- so a stage works on a square root of its own: in
// d_bsqrt, which the call's setup has reserved for nc chains, as it has cleared the status word.  Then get_terminf of those chains into
// d_ainf / d_binf, unless the caller gave terminators (d_ainf == nullptr).
int resident_block_prologue(rsrec_t* h, size_t c0, size_t nc, int lld, double* d_ainf, double* d_binf) {
    const size_t cel = (size_t)lld * BLK;
    double2* dBs = h->d_bsqrt.as<double2>();
    HIPCK(h, hipMemcpyAsync(dBs, h->d_coefB.as<double2>() + c0 * cel, nc * cel * sizeof(double2), hipMemcpyDeviceToDevice, h->stream));
    k_zsqr<<<(unsigned)(nc * lld), 256, 0, h->stream>>>(dBs, h->d_status.as<int>());
    if (!d_ainf) return RSREC_OK;
    return launch_terminator(h, (int)nc, lld, h->d_coefA.as<double2>() + c0 * cel, dBs, d_ainf, d_binf);
}

}  // namespace

// recursion%get_terminf (recursion.f90:2092-2135) for `nsites` sites, host arrays in and out.
extern "C" int rsrec_terminator(rsrec_t* h, int nsites, int lld, const double* a_b, const double* b_sqrt, double* a_inf, double* b_inf,
                                double* a_inf0, double* b_inf0) {
    if (!h) return RSREC_ERR_ARG;
    if (nsites < 0 || lld < 2 || (nsites > 0 && (!a_b || !b_sqrt || !a_inf || !b_inf))) return fail(h, RSREC_ERR_ARG, "rsrec_terminator: bad argument");
    if (nsites == 0) return RSREC_OK;
    HIPCK(h, hipSetDevice(h->device));
    const size_t cbytes = (size_t)nsites * lld * BLK * sizeof(double2), tbytes = (size_t)nsites * BLK * sizeof(double);
    release_kubo_buffers(h, true, true);
    HIPCK(h, h->d_green_in.reserve(2 * cbytes));
    HIPCK(h, h->d_term.reserve(2 * tbytes + 2 * (size_t)nsites * sizeof(double)));
    double2* d_ab = h->d_green_in.as<double2>();
    double2* d_bs = d_ab + (size_t)nsites * lld * BLK;
    double* d_ai = h->d_term.as<double>();
    double* d_bi = d_ai + (size_t)nsites * BLK;
    double* d_a0 = d_bi + (size_t)nsites * BLK;
    XFER(xfer_h2d(h, d_ab, a_b, cbytes));
    XFER(xfer_h2d(h, d_bs, b_sqrt, cbytes));
    reset_timing(h);
    hipEvent_t e0 = next_event(h);
    int rc = launch_terminator(h, nsites, lld, d_ab, d_bs, d_ai, d_bi);
    if (rc) return rc;
    k_terminator_means<<<(nsites + 63) / 64, 64, 0, h->stream>>>(d_ai, d_bi, d_a0, d_a0 + nsites, nsites);
    hipEvent_t e1 = next_event(h);
    XFER(xfer_d2h(h, a_inf, d_ai, tbytes));
    XFER(xfer_d2h(h, b_inf, d_bi, tbytes));
    if (a_inf0) XFER(xfer_d2h(h, a_inf0, d_a0, (size_t)nsites * sizeof(double)));
    if (b_inf0) XFER(xfer_d2h(h, b_inf0, d_a0 + nsites, (size_t)nsites * sizeof(double)));
    HIPCK(h, hipStreamSynchronize(h->stream));
    h->t_total_ms = h->t_hop_ms = ev_ms(e0, e1);
    return RSREC_OK;
}

// dos%density for every (site, direction) of a scalar-recursion run (density_of_states.f90:248-363, bprldos :370-404; called by
// green%sgreen, green.f90:661): a, b2 (llmax, 18, nsites, nmdir) as recursion%a / %b2 hold them, dw_l, cshi (18, nsites) = the potential
// parameters of the sites' atoms, ene (npts) -> tdens (18, npts, nsites, nmdir).
extern "C" int rsrec_scalar_density(rsrec_t* h, int nsites, int nmdir, int llmax, int lld, const double* a, const double* b2, int npts, const double* ene,
                                    const double* dw_l, const double* cshi, double* tdens) {
    if (!h) return RSREC_ERR_ARG;
    if (nsites < 0 || nmdir < 1 || lld < 2 || lld > llmax || npts < 0 || ((nsites > 0 && npts > 0) && (!a || !b2 || !ene || !dw_l || !cshi || !tdens)))
        return fail(h, RSREC_ERR_ARG, "rsrec_scalar_density: bad argument");
    if (nsites == 0 || npts == 0) return RSREC_OK;
    HIPCK(h, hipSetDevice(h->device));
    const int nchain = NB * nsites * nmdir;
    const size_t cb = (size_t)nchain * llmax * sizeof(double), pb = (size_t)NB * nsites * sizeof(double), eb = (size_t)npts * sizeof(double),
                 gb = 2 * (size_t)nchain * sizeof(double), tb = (size_t)nchain * npts * sizeof(double);
    release_kubo_buffers(h, true, true);
    HIPCK(h, h->d_green_in.reserve(2 * cb + 2 * pb + eb + gb));
    HIPCK(h, h->d_green_out.reserve(tb));
    double* d_a = h->d_green_in.as<double>();
    double* d_b = d_a + (size_t)nchain * llmax;
    double* d_dw = d_b + (size_t)nchain * llmax;
    double* d_cs = d_dw + (size_t)NB * nsites;
    double* d_en = d_cs + (size_t)NB * nsites;
    double* d_ed = d_en + npts;
    double* d_t = h->d_green_out.as<double>();
    XFER(xfer_h2d(h, d_a, a, cb));
    XFER(xfer_h2d(h, d_b, b2, cb));
    XFER(xfer_h2d(h, d_dw, dw_l, pb));
    XFER(xfer_h2d(h, d_cs, cshi, pb));
    XFER(xfer_h2d(h, d_en, ene, eb));
    reset_timing(h);
    hipEvent_t e0 = next_event(h);
    // one LDS column of 2 lld doubles per thread: as many threads per workgroup as 64 KB hold (64 up to lld = 64, one at lld = 4096)
    const int T = (int)std::max<size_t>(1, std::min<size_t>(64, (64 * 1024) / (2 * (size_t)lld * sizeof(double))));
    const size_t lds = 2 * (size_t)lld * T * sizeof(double);
    if (lds > 64 * 1024) return fail(h, RSREC_ERR_ARG, "rsrec_scalar_density: lld = %d too deep for the band-edge kernel", lld);
    k_scalar_edges<<<(nchain + T - 1) / T, T, lds, h->stream>>>(lld, llmax, nchain, d_a, d_b, d_ed);
    k_scalar_density<<<dim3((npts + 127) / 128, nchain), 128, 0, h->stream>>>(lld, llmax, npts, nsites, d_a, d_b, d_en, d_dw, d_cs, d_ed, d_t);
    HIPCK(h, hipGetLastError());
    hipEvent_t e1 = next_event(h);
    XFER(xfer_d2h(h, tdens, d_t, tb));
    HIPCK(h, hipStreamSynchronize(h->stream));
    h->t_total_ms = h->t_hop_ms = ev_ms(e0, e1);
    return RSREC_OK;
}

namespace {

// The Jackson kernel of green%chebyshev_green (math.f90:1641-1655; real(ll) is a default-REAL conversion, exact for these small
// integers) with mu_ng(:,:,2:) *= 2 (green.f90:1074) folded in.
std::vector<double> chebyshev_green_kernel(int nm) {
    std::vector<double> kern(nm);
    const double pi = 3.14159265358979323846;
    for (int ll = 1; ll <= nm; ++ll) {
        const double theta = pi * ((double)ll - 1.0) / ((double)nm + 1.0);
        kern[ll - 1] = (((double)nm - ((double)ll - 1.0) + 1.0) * cos(theta) + sin(theta) / tan(pi / ((double)nm + 1.0))) / ((double)nm + 1.0);
        if (ll > 1) kern[ll - 1] *= 2.0;
    }
    return kern;
}

// Scale and shift of green%chebyshev_green as the reference writes them (default-REAL literals 2 and 0.3, green.f90:1046-1047)
void chebyshev_green_scaling(double energy_min, double energy_max, double& a, double& b) {
    a = (energy_max - energy_min) / (double)(2.0f - 0.3f);
    b = (energy_max + energy_min) / 2;
}

}  // namespace

// green%chebyshev_green (green.f90:1030-1108): g0 from the Chebyshev moments of every site.
extern "C" int rsrec_chebyshev_green(rsrec_t* h, int nsites, int lld, int nen, const double* ene, double energy_min, double energy_max,
                                     const double* mu_n, double* g0) {
    if (!h) return RSREC_ERR_ARG;
    if (nsites < 0 || lld < 1 || nen < 0 || (nsites > 0 && nen > 0 && (!ene || !mu_n || !g0))) return fail(h, RSREC_ERR_ARG, "rsrec_chebyshev_green: bad argument");
    if (nsites == 0 || nen == 0) return RSREC_OK;
    HIPCK(h, hipSetDevice(h->device));
    const int nm = 2 * lld + 2;
    double a, b;
    chebyshev_green_scaling(energy_min, energy_max, a, b);
    const std::vector<double> kern = chebyshev_green_kernel(nm);
    const size_t mbytes = (size_t)nm * BLK * sizeof(double2), gbytes = (size_t)nen * BLK * sizeof(double2);
    const int super = (int)std::max<size_t>(1, std::min<size_t>((size_t)nsites, ((size_t)4 << 30) / mbytes));
    release_kubo_buffers(h, true, true);
    HIPCK(h, h->d_green_in.reserve((size_t)super * mbytes + (size_t)(nen + nm) * sizeof(double)));
    double* d_ene = static_cast<double*>(h->d_green_in.p);
    double* d_kern = d_ene + nen;
    double2* d_mu = reinterpret_cast<double2*>(d_kern + nm);
    XFER(xfer_h2d(h, d_ene, ene, (size_t)nen * sizeof(double)));
    XFER(xfer_h2d(h, d_kern, kern.data(), (size_t)nm * sizeof(double)));
    reset_timing(h);
    hipEvent_t ev0 = next_event(h);
    for (int u0 = 0; u0 < nsites; u0 += super) {
        const int nu = std::min(super, nsites - u0);
        XFER(xfer_h2d(h, d_mu, mu_n + (size_t)u0 * nm * BLK * 2, (size_t)nu * mbytes));
        XFER(green_pipeline(h, nu, gbytes, g0 + (size_t)u0 * nen * BLK * 2, [&](int s0, int ns, char* out) {
            k_chebyshev_green<<<dim3(nen, ns), 256, (size_t)nm * sizeof(double2), h->stream>>>(nm, nen, d_ene, a, b, d_kern, d_mu + (size_t)s0 * nm * BLK, reinterpret_cast<double2*>(out));
        }));
    }
    hipEvent_t ev1 = next_event(h);
    HIPCK(h, hipStreamSynchronize(h->stream));
    h->t_total_ms = ev_ms(ev0, ev1);
    return RSREC_OK;
}

namespace {

// Call setup shared by the stages that run on the on-site chains the last recursion left on the device (rsrec_block_ldos,
// rsrec_chebyshev_ldos, rsrec_block_spectra, rsrec_chebyshev_spectra), as PairCall is for the calls on pairs:
//   site_stage_begin  the residency and site-range rules, the device, the stage's scratch with ene (| the Chebyshev kernel weights)
//                     behind it, the buffers and the cleared status word of the block prologue or the Chebyshev scaling;
//   (the stage's own uploads and LDS opt-in, outside the timed span)
//   site_stage_open   the timed span opens; the block prologue;
//   (the stage's kernels and delivery)
//   site_stage_end    the status word, the stream, the timing.
struct SiteStage {
    int kind, n, lld, nm;                          // 1 = block Lanczos, 2 = Chebyshev; sites; depth; moments per site
    const double2 *sa, *sb;                        // a_b and the stage's sqrt(b2_b), or mu_n and nullptr
    double *ta, *tb;                               // terminators (kind 1)
    double ca, cb;                                 // chebyshev_green's scaling (kind 2)
    double *d_out, *d_ene, *d_kern;                // the scratch (per_site doubles per site), the energies, the Chebyshev kernel weights (kind 2)
    hipEvent_t e0, k0;                             // the opening event, the event behind the prologue (e0 itself where there is none)
};

int site_stage_begin(rsrec_t* h, SiteStage& S, const char* who, int kind, int nen, const double* ene, double energy_min, double energy_max,
                     int site_offset, int nsites_total, DevBuf& scratch, size_t per_site) {
    if (nen < 1 || !ene || site_offset < 0) return fail(h, RSREC_ERR_ARG, "%s: bad argument", who);
    if (h->res_kind != kind)
        return fail(h, RSREC_ERR_ARG, kind == 1 ? "%s: no block-Lanczos coefficients resident (call rsrec_block_lanczos first)" : "%s: no Chebyshev moments resident (call rsrec_chebyshev first)", who);
    if (site_offset + h->res_n > nsites_total) return fail(h, RSREC_ERR_ARG, "%s: sites %d..%d outside 1..%d", who, site_offset + 1, site_offset + h->res_n, nsites_total);
    HIPCK(h, hipSetDevice(h->device));
    S.kind = kind; S.n = h->res_n; S.lld = h->res_lld; S.nm = 2 * h->res_lld + 2;
    const size_t n = (size_t)S.n;
    release_kubo_buffers(h, true, true);
    HIPCK(h, scratch.reserve((per_site * n + (size_t)nen + (kind == 2 ? S.nm : 0)) * sizeof(double)));
    S.d_out = scratch.as<double>();
    S.d_ene = S.d_out + per_site * n;
    S.d_kern = S.d_ene + nen;
    if (kind == 1) {
        HIPCK(h, h->d_bsqrt.reserve(n * S.lld * BLK * sizeof(double2)));
        HIPCK(h, h->d_term.reserve(2 * n * BLK * sizeof(double) + 2 * n * sizeof(double)));
        HIPCK(h, h->d_status.reserve(64));
        HIPCK(h, hipMemsetAsync(h->d_status.p, 0, 64, h->stream));
        S.sa = h->d_coefA.as<double2>(); S.sb = h->d_bsqrt.as<double2>();
        S.ta = h->d_term.as<double>(); S.tb = S.ta + n * BLK;
    } else {
        chebyshev_green_scaling(energy_min, energy_max, S.ca, S.cb);
        const std::vector<double> kern = chebyshev_green_kernel(S.nm);
        XFER(xfer_h2d(h, S.d_kern, kern.data(), (size_t)S.nm * sizeof(double)));
        S.sa = h->d_mu.as<double2>(); S.sb = nullptr;
        S.ta = S.tb = nullptr;
    }
    return xfer_h2d(h, S.d_ene, ene, (size_t)nen * sizeof(double));
}

int site_stage_open(rsrec_t* h, SiteStage& S) {
    reset_timing(h);
    S.e0 = S.k0 = next_event(h);
    if (S.kind == 2) return RSREC_OK;
    XFER(resident_block_prologue(h, 0, (size_t)S.n, S.lld, S.ta, S.tb));
    S.k0 = next_event(h);
    return RSREC_OK;
}

// e1: where the stage's timed span ends; k0, k1: what it reports as hop
int site_stage_end(rsrec_t* h, const SiteStage& S, hipEvent_t k0, hipEvent_t k1, hipEvent_t e1) {
    int rc = RSREC_OK;
    if (S.kind == 1) rc = finish_status(h);
    else HIPCK(h, hipStreamSynchronize(h->stream));
    finish_timing(h, S.e0, e1, {{k0, k1}});
    return rc;
}

// The way out of Im g0_jj [site][nen][18] of the rank's sites: the zero-padded images dosial | dosia | dtot of calculate_fermi's reduction,
// formed in the caller's arrays if those are device memory, else in d_ldos and downloaded.  reduced: the event behind the reduction (the
// timed span of an LDOS stage ends there, before the downloads).
int ldos_deliver(rsrec_t* h, const double* d_gim, int n, int nen, int site_offset, int nsites_total, double* dtot, double* dosia, double* dosial,
                 hipEvent_t& reduced) {
    const size_t nial = (size_t)nsites_total * NB * nen, nia = (size_t)nsites_total * nen;
    const bool dev = is_device_ptr(dtot) && is_device_ptr(dosia) && is_device_ptr(dosial);
    if (!dev) HIPCK(h, h->d_ldos.reserve((nial + nia + (size_t)nen) * sizeof(double)));
    double* o_dosial = dev ? dosial : h->d_ldos.as<double>();
    double* o_dosia = dev ? dosia : o_dosial + nial;
    double* o_dtot = dev ? dtot : o_dosia + nia;
    k_ldos_finish<<<(nen + 63) / 64, 64, 0, h->stream>>>(d_gim, n, nen, site_offset, nsites_total, o_dosial, o_dosia, o_dtot);
    HIPCK(h, hipGetLastError());
    reduced = next_event(h);
    if (dev) return RSREC_OK;
    XFER(xfer_d2h(h, dosial, o_dosial, nial * sizeof(double)));
    XFER(xfer_d2h(h, dosia, o_dosia, nia * sizeof(double)));
    return xfer_d2h(h, dtot, o_dtot, (size_t)nen * sizeof(double));
}

// what rsrec_block_spectra and rsrec_chebyshev_spectra share beside the stage setup: the rules for the operators, the way out of the compact
// block spec[site][nen][nop] of the rank's sites into the caller's zero-padded image
int spectra_check(rsrec_t* h, const char* who, int nop, const double* ops, const double* spec) {
    if (!ops || !spec) return fail(h, RSREC_ERR_ARG, "%s: bad argument", who);
    if (nop < 1 || nop > SPECTRA_MAX_OPS) return fail(h, RSREC_ERR_ARG, "%s: nop = %d outside 1..%d", who, nop, SPECTRA_MAX_OPS);
    return RSREC_OK;
}

int spectra_deliver(rsrec_t* h, const double* d_spec, size_t per_site, int n, int site_offset, int nsites_total, double* spec) {
    const size_t lo = per_site * site_offset, nfill = per_site * n, total = per_site * nsites_total;
    if (is_device_ptr(spec)) {
        k_spectra_image<<<(unsigned)std::min<size_t>((total + 255) / 256, 4096), 256, 0, h->stream>>>(d_spec, lo, nfill, total, spec);
        HIPCK(h, hipGetLastError());
        return RSREC_OK;
    }
    memset(spec, 0, lo * sizeof(double));
    memset(spec + lo + nfill, 0, (total - lo - nfill) * sizeof(double));
    return xfer_d2h(h, spec + lo, d_spec, nfill * sizeof(double));
}

}  // namespace

// The whole LDOS stage for the sites of the last rsrec_block_lanczos call, from the coefficients it left on the device:
// zsqr (recursion.f90:1980) -> get_terminf (:2092) -> bgreen (green.f90:1191) -> the reduction of calculate_fermi (bands.f90:258-268).
// Only the densities of states leave the GPU (18 doubles per site and energy instead of 648).
extern "C" int rsrec_block_ldos(rsrec_t* h, int nen, const double* ene, double eta_re, double eta_im, int sym_term, int site_offset, int nsites_total,
                                double* dtot, double* dosia, double* dosial, double* a_inf_out, double* b_inf_out) {
    if (!h) return RSREC_ERR_ARG;
    if (!dtot || !dosia || !dosial) return fail(h, RSREC_ERR_ARG, "rsrec_block_ldos: bad argument");
    SiteStage S;
    XFER(site_stage_begin(h, S, "rsrec_block_ldos", 1, nen, ene, 0.0, 0.0, site_offset, nsites_total, h->d_gim, (size_t)nen * NB));
    h->n_ldos_calls++;
    XFER(site_stage_open(h, S));
    {
        const dim3 grid((nen + GREEN_WAVES - 1) / GREEN_WAVES, S.n);
        k_block_green<true><<<grid, GREEN_WAVES * 64, 0, h->stream>>>(S.lld, nen, S.d_ene, eta_re, eta_im, sym_term, S.ta, S.tb, S.sa, S.sb, nullptr, S.d_out);
    }
    hipEvent_t k1 = next_event(h), e1 = nullptr;
    XFER(ldos_deliver(h, S.d_out, S.n, nen, site_offset, nsites_total, dtot, dosia, dosial, e1));
    if (a_inf_out) XFER(xfer_d2h(h, a_inf_out, S.ta, (size_t)S.n * BLK * sizeof(double)));
    if (b_inf_out) XFER(xfer_d2h(h, b_inf_out, S.tb, (size_t)S.n * BLK * sizeof(double)));
    return site_stage_end(h, S, S.k0, k1, e1);        // hop: the Green kernel alone; rest: zsqr + terminator + reduction
}

// The LDOS stage for the sites of the last rsrec_chebyshev call, from the moments it left on the device: the diagonal of
// green%chebyshev_green (green.f90:1030-1108) -> the reduction of calculate_fermi (bands.f90:258-268).  Neither the moments nor a g0
// cross PCIe: the energy mesh and the nm kernel weights go up, 18 doubles per site and energy come back.
extern "C" int rsrec_chebyshev_ldos(rsrec_t* h, int nen, const double* ene, double energy_min, double energy_max, int site_offset, int nsites_total,
                                    double* dtot, double* dosia, double* dosial) {
    if (!h) return RSREC_ERR_ARG;
    if (!dtot || !dosia || !dosial) return fail(h, RSREC_ERR_ARG, "rsrec_chebyshev_ldos: bad argument");
    SiteStage S;
    XFER(site_stage_begin(h, S, "rsrec_chebyshev_ldos", 2, nen, ene, energy_min, energy_max, site_offset, nsites_total, h->d_gim, (size_t)nen * NB));
    const size_t lds = (size_t)S.nm * NB * sizeof(double2);          // the diagonal moments of one site (29 KB at lld = 50)
    if (lds > (size_t)150 * 1024) return fail(h, RSREC_ERR_ARG, "rsrec_chebyshev_ldos: lld = %d too deep for the LDS staging", S.lld);
    XFER(lds_opt_in(h, reinterpret_cast<const void*>(k_chebyshev_ldos), lds, h->cheb_ldos_lds));
    h->n_ldos_calls++;
    XFER(site_stage_open(h, S));
    {
        const dim3 grid((nen + CHEB_LDOS_TILE - 1) / CHEB_LDOS_TILE, S.n);
        k_chebyshev_ldos<<<grid, CHEB_LDOS_TILE, lds, h->stream>>>(S.nm, nen, S.d_ene, S.ca, S.cb, S.d_kern, S.sa, S.d_out);
    }
    hipEvent_t k1 = next_event(h), e1 = nullptr;
    XFER(ldos_deliver(h, S.d_out, S.n, nen, site_offset, nsites_total, dtot, dosia, dosial, e1));
    return site_stage_end(h, S, S.e0, k1, e1);        // hop: from the opening event through k_chebyshev_ldos; rest: the reduction
}

// Im Tr(O_k g0) of green%bgreen for the sites of the last rsrec_block_lanczos call, from the coefficients it left on the device:
// zsqr -> get_terminf -> the continued fraction of bgreen with the contraction as its epilogue.  No g0 leaves the kernel.
extern "C" int rsrec_block_spectra(rsrec_t* h, int nop, const double* ops, int nen, const double* ene, double eta_re, double eta_im, int sym_term,
                                   int site_offset, int nsites_total, double* spec) {
    if (!h) return RSREC_ERR_ARG;
    XFER(spectra_check(h, "rsrec_block_spectra", nop, ops, spec));
    h->spec_res.nop = 0;
    const size_t obytes = (size_t)nop * BLK * sizeof(double2), per_site = (size_t)nop * nen;
    SiteStage S;
    XFER(site_stage_begin(h, S, "rsrec_block_spectra", 1, nen, ene, 0.0, 0.0, site_offset, nsites_total, h->d_spec, per_site));
    const double2* d_ops = reinterpret_cast<const double2*>(ops);
    if (!is_device_ptr(ops)) {
        HIPCK(h, h->d_ops.reserve(obytes));
        XFER(xfer_h2d(h, h->d_ops.p, ops, obytes));
        d_ops = h->d_ops.as<double2>();
    }
    XFER(site_stage_open(h, S));
    {
        const dim3 grid((nen + GREEN_WAVES - 1) / GREEN_WAVES, S.n);
        k_block_spectra<<<grid, GREEN_WAVES * 64, 0, h->stream>>>(S.lld, nen, S.d_ene, eta_re, eta_im, sym_term, S.ta, S.tb, S.sa, S.sb, nop, d_ops, S.d_out);
    }
    HIPCK(h, hipGetLastError());
    hipEvent_t k1 = next_event(h);
    XFER(spectra_deliver(h, S.d_out, per_site, S.n, site_offset, nsites_total, spec));
    XFER(site_stage_end(h, S, S.k0, k1, next_event(h)));    // hop: the Green kernel with its epilogue; rest: zsqr + terminator + delivery
    h->spec_res.nop = nop; h->spec_res.nen = nen; h->spec_res.n = S.n; h->spec_res.site_offset = site_offset; h->spec_res.nsites_total = nsites_total;
    return RSREC_OK;
}

// Im Tr(O_k g0) of green%chebyshev_green for the sites of the last rsrec_chebyshev call, from the moments it left on the device:
// t(k, i) = Tr(O_k mu_i) once per site, then the energy sum of rsrec_chebyshev_ldos on t.
extern "C" int rsrec_chebyshev_spectra(rsrec_t* h, int nop, const double* ops, int nen, const double* ene, double energy_min, double energy_max,
                                       int site_offset, int nsites_total, double* spec) {
    if (!h) return RSREC_ERR_ARG;
    XFER(spectra_check(h, "rsrec_chebyshev_spectra", nop, ops, spec));
    h->spec_res.nop = 0;
    const size_t obytes = (size_t)nop * BLK * sizeof(double2), per_site = (size_t)nop * nen;
    SiteStage S;
    XFER(site_stage_begin(h, S, "rsrec_chebyshev_spectra", 2, nen, ene, energy_min, energy_max, site_offset, nsites_total, h->d_spec, per_site));
    const size_t lds = (size_t)S.nm * nop * sizeof(double2);          // the operator traces of one site (24 KB at lld = 50, 15 operators)
    if (lds > (size_t)150 * 1024) return fail(h, RSREC_ERR_ARG, "rsrec_chebyshev_spectra: lld = %d with %d operators too deep for the LDS staging", S.lld, nop);
    XFER(lds_opt_in(h, reinterpret_cast<const void*>(k_chebyshev_spectra), lds, h->cheb_spec_lds));
    HIPCK(h, h->d_ops.reserve(obytes + (size_t)S.n * lds));           // the operators (if they are host memory) | their traces with every moment of every site
    const double2* d_ops = reinterpret_cast<const double2*>(ops);
    if (!is_device_ptr(ops)) {
        XFER(xfer_h2d(h, h->d_ops.p, ops, obytes));
        d_ops = h->d_ops.as<double2>();
    }
    double2* d_t = reinterpret_cast<double2*>(static_cast<char*>(h->d_ops.p) + obytes);
    XFER(site_stage_open(h, S));
    k_chebyshev_optrace<<<dim3(S.nm, S.n), 64, 0, h->stream>>>(S.nm, nop, d_ops, S.sa, d_t);
    hipEvent_t k0 = next_event(h);
    {
        const dim3 grid((nen + CHEB_LDOS_TILE - 1) / CHEB_LDOS_TILE, S.n);
        k_chebyshev_spectra<<<grid, CHEB_LDOS_TILE, lds, h->stream>>>(S.nm, nop, nen, S.d_ene, S.ca, S.cb, S.d_kern, d_t, S.d_out);
    }
    HIPCK(h, hipGetLastError());
    hipEvent_t k1 = next_event(h);
    XFER(spectra_deliver(h, S.d_out, per_site, S.n, site_offset, nsites_total, spec));
    XFER(site_stage_end(h, S, k0, k1, next_event(h)));      // hop: the energy sum alone; rest: the operator traces + delivery
    h->spec_res.nop = nop; h->spec_res.nen = nen; h->spec_res.n = S.n; h->spec_res.site_offset = site_offset; h->spec_res.nsites_total = nsites_total;
    return RSREC_OK;
}
// The integrals behind the spectra (kernels_moments.hpp): the series y = comb . spec of every site, their cumulative Simpson integrals up to
// every mesh energy (T = 0, a prefix of the rule) and their simpson_m integrals of orders 0, 1, 2 up to the Fermi level.  Reads no chains:
// spec is the caller's image or the one the last spectra call left in d_spec, so no SiteStage -- only its image rules (site_offset,
// nsites_total, host or device memory) and its timing apply.
extern "C" int rsrec_spectra_integrals(rsrec_t* h, int nop, const double* spec, int nser, const double* comb, int nen, const double* ene, int nv1,
                                       int nv1_fermi, double edel, double e1, double fermi, int nsites, int site_offset, int nsites_total,
                                       double* mom, double* cum) {
    const char* who = "rsrec_spectra_integrals";
    if (!h) return RSREC_ERR_ARG;
    if (!ene) return fail(h, RSREC_ERR_ARG, "%s: bad argument: ene is NULL", who);
    if (!mom && !cum) return fail(h, RSREC_ERR_ARG, "%s: bad argument: mom and cum are both NULL", who);
    if (nsites < 1 || site_offset < 0) return fail(h, RSREC_ERR_ARG, "%s: bad argument: nsites = %d, site_offset = %d", who, nsites, site_offset);
    if (nv1 < 1) return fail(h, RSREC_ERR_ARG, "%s: bad argument: nv1 = %d", who, nv1);
    if (nop < 1 || nop > SPECTRA_MAX_OPS) return fail(h, RSREC_ERR_ARG, "%s: nop = %d outside 1..%d", who, nop, SPECTRA_MAX_OPS);
    if (nser < 1 || nser > MOMENT_MAX_SERIES) return fail(h, RSREC_ERR_ARG, "%s: nser = %d outside 1..%d", who, nser, MOMENT_MAX_SERIES);
    if (!comb && nser != nop) return fail(h, RSREC_ERR_ARG, "%s: without comb the series are the %d rows, not nser = %d", who, nop, nser);
    if (site_offset + nsites > nsites_total) return fail(h, RSREC_ERR_ARG, "%s: sites %d..%d outside 1..%d", who, site_offset + 1, site_offset + nsites, nsites_total);
    if (nen < nv1 + 9) return fail(h, RSREC_ERR_ARG, "%s: nen = %d below nv1 + 9 = %d, the points the rule reads", who, nen, nv1 + 9);
    if (nv1_fermi < 1 || nv1_fermi + 2 > nen) return fail(h, RSREC_ERR_ARG, "%s: nv1_fermi = %d outside 1..nen - 2 = %d", who, nv1_fermi, nen - 2);
    if (!std::isfinite(edel) || !std::isfinite(e1) || !std::isfinite(fermi)) return fail(h, RSREC_ERR_ARG, "%s: edel, e1 and fermi must be finite", who);
    // the prefix form rests on Fermi weights that are exactly 1, 0.5, 0: kBT = 1e-15 against an ascending mesh of step > 1e-12
    for (int k = 0; k + 1 < nen; ++k)
        if (!(ene[k + 1] - ene[k] > 1.0e-12)) return fail(h, RSREC_ERR_ARG, "%s: the mesh must ascend by more than 1e-12 per point (ene(%d), ene(%d))", who, k + 1, k + 2);
    if (!spec) {
        const auto& R = h->spec_res;
        if (R.nop == 0) return fail(h, RSREC_ERR_ARG, "%s: no spectra image resident (call rsrec_block_spectra / rsrec_chebyshev_spectra first, or pass spec)", who);
        if (R.nop != nop || R.nen != nen || R.n != nsites || R.site_offset != site_offset || R.nsites_total != nsites_total)
            return fail(h, RSREC_ERR_ARG, "%s: the resident image is (%d, %d) for sites %d..%d of %d, the call asks for (%d, %d) for sites %d..%d of %d", who, R.nop, R.nen,
                        R.site_offset + 1, R.site_offset + R.n, R.nsites_total, nop, nen, site_offset + 1, site_offset + nsites, nsites_total);
    }
    HIPCK(h, hipSetDevice(h->device));
    const size_t n = (size_t)nsites, slab = (size_t)nop * nen * n, ncomb = comb ? (size_t)nop * nser * n : 0;
    const int ntrip = (nv1 + 9) / 2;
    const bool spec_up = spec && !is_device_ptr(spec), comb_up = comb && !is_device_ptr(comb);
    const bool cum_dev = cum && is_device_ptr(cum), mom_dev = mom && is_device_ptr(mom);
    const size_t ncum = (size_t)nser * nen * nsites_total, nmom = (size_t)3 * nser * nsites_total;
    // the scratch: uploaded spec | uploaded comb | series | running sums | mesh | cum image | mom image (each only where it is needed)
    const size_t o_comb = spec_up ? slab : 0, o_y = o_comb + (comb_up ? ncomb : 0), o_p = o_y + (comb ? (size_t)nser * nen * n : 0);
    const size_t o_ene = o_p + (cum ? (size_t)nser * (ntrip + 1) * n : 0), o_cum = o_ene + nen, o_mom = o_cum + (cum && !cum_dev ? ncum : 0);
    HIPCK(h, h->d_mint.reserve((o_mom + (mom && !mom_dev ? nmom : 0)) * sizeof(double)));
    double* W = h->d_mint.as<double>();
    const double* d_spec = !spec ? h->d_spec.as<double>() : spec + (size_t)site_offset * nop * nen;
    if (spec_up) { XFER(xfer_h2d(h, W, d_spec, slab * sizeof(double))); d_spec = W; }
    const double* d_comb = comb;
    if (comb_up) { XFER(xfer_h2d(h, W + o_comb, comb, ncomb * sizeof(double))); d_comb = W + o_comb; }
    double* d_ene = W + o_ene;
    XFER(xfer_h2d(h, d_ene, ene, (size_t)nen * sizeof(double)));
    reset_timing(h);
    hipEvent_t e0 = next_event(h);
    const unsigned gx = (unsigned)(((size_t)nen * nser + MI_WIDTH - 1) / MI_WIDTH);
    const double* d_y = d_spec;                      // without comb the series are the rows where they lie
    int ld = nop;
    if (comb) {
        k_moment_series<<<dim3(gx, nsites), MI_WIDTH, 0, h->stream>>>(nop, nser, nen, d_spec, d_comb, W + o_y);
        d_y = W + o_y; ld = nser;
    }
    double* o_cum_p = cum_dev ? cum : W + o_cum;
    double* o_mom_p = mom_dev ? mom : W + o_mom;
    if (cum) {
        k_moment_prefix<<<(unsigned)((nser * n + MI_WIDTH - 1) / MI_WIDTH), MI_WIDTH, 0, h->stream>>>(nser, ld, nen, ntrip, nsites, d_y, W + o_p);
        k_moment_cum<<<dim3(gx, nsites_total), MI_WIDTH, 0, h->stream>>>(nser, ld, nen, nv1, site_offset, nsites, d_ene, d_y, W + o_p, o_cum_p);
    }
    if (mom)
        k_moment_fermi<<<(unsigned)((nmom + MI_WIDTH - 1) / MI_WIDTH), MI_WIDTH, 0, h->stream>>>(nser, ld, nen, nv1_fermi, edel, e1, fermi, site_offset, nsites,
                                                                                              nsites_total, d_ene, d_y, o_mom_p);
    HIPCK(h, hipGetLastError());
    hipEvent_t e1v = next_event(h);
    if (cum && !cum_dev) XFER(xfer_d2h(h, cum, o_cum_p, ncum * sizeof(double)));
    if (mom && !mom_dev) XFER(xfer_d2h(h, mom, o_mom_p, nmom * sizeof(double)));
    HIPCK(h, hipStreamSynchronize(h->stream));
    finish_timing(h, e0, e1v, {});
    return RSREC_OK;
}

namespace {

__global__ void k_copy_d(const double* __restrict__ src, double* __restrict__ dst, size_t n) {
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) dst[k] = src[k];
}

// device -> caller array (host or device memory; a device array may belong to another HIP runtime of the process: copied by a kernel)
int xc_deliver(rsrec_t* h, double* dst, const double* src, size_t n) {
    if (n == 0) return RSREC_OK;
    if (is_device_ptr(dst)) {
        k_copy_d<<<(unsigned)std::min<size_t>((n + 255) / 256, 4096), 256, 0, h->stream>>>(src, dst, n);
        HIPCK(h, hipGetLastError());
        return RSREC_OK;
    }
    return xfer_d2h(h, dst, src, n * sizeof(double));
}

// caller array -> device: a device array is read where it lies, a host array is staged in `stage`
int xc_fetch(rsrec_t* h, const double* src, double* stage, size_t n, const double** out) {
    if (is_device_ptr(src)) { *out = src; return RSREC_OK; }
    *out = stage;
    return xfer_h2d(h, stage, src, n * sizeof(double));
}

}  // namespace

namespace {

// Call setup shared by the entry points that run a kernel per (pair, energy) on the four chains of every pair (rsrec_exchange,
// rsrec_damping, rsrec_exchange_contour, rsrec_exchange_aux, rsrec_spin_lattice) or, with per = 1, per (site, point) on the one chain of every site (rsrec_contour_occupation): the coefficient-source rules, the compaction of resident i == j pairs, the chunking over pairs and the device buffers.
//   d_green_in : ene | the call's own inputs (fixed_in) | same | cbase | a_b (or mu_n) | b_sqrt | a_inf (or the Chebyshev kernel) | b_inf |
//                the chunk's own inputs (chunk_in per pair)                                       (chunk-sized from a_b on)
//   d_green_out: the rows of the chunk (row_doubles per pair) | the call's own outputs (fixed_out) | chunk_out per pair
struct PairCall {
    const char* who;
    int kind, npairs, lld, nen, nm, P;             // P: pairs per chunk
    int per;                                       // chain slots per pair: 4, or 1 when the "pairs" are on-site chains (rsrec_contour_occupation)
    bool resident, compact;
    std::vector<int> cbase;                        // first chain of every pair
    size_t cel;                                    // complex elements per chain (each of a_b, b_sqrt / mu_n)
    double ca, cb;                                 // chebyshev_green_ij's scaling
    const double *a_inf, *b_inf, *coef_a, *coef_b;
    double *din, *d_ene, *d_fixed_in, *d_chunk_in, *d_rows, *d_fixed_out, *d_chunk_out;
    int *d_same, *d_cb;
    size_t off_ab, off_bs, off_ai, off_bi;
    size_t row_doubles, fixed_out, chunk_out;      // doubles of the rows of one pair, of the call's own outputs, of the chunk outputs of one pair
};

// the chains of one chunk, as the kernels read them
struct PairChunk {
    int np, c0;                                    // pairs, first chain
    const double2 *sa, *sb;                        // a_b and b_sqrt, or mu_n and nullptr
    const double *ta, *tb;                         // terminators (kind 0), or the Chebyshev kernel weights and nullptr
};

size_t even(size_t n) { return (n + 1) & ~(size_t)1; }

int pair_call_begin(rsrec_t* h, PairCall& c, const char* who, int kind, int npairs, const int32_t* same, int lld, int nen, const double* ene,
                    double energy_min, double energy_max, const double* a_inf, const double* b_inf, const double* coef_a, const double* coef_b,
                    size_t row_doubles, size_t fixed_in, size_t chunk_in, size_t fixed_out, size_t chunk_out, int per = 4, int group = 1) {
    if (kind < 0 || kind > 1) return fail(h, RSREC_ERR_ARG, "%s: kind %d is neither 0 (block) nor 1 (Chebyshev)", who, kind);
    if ((a_inf == nullptr) != (b_inf == nullptr)) return fail(h, RSREC_ERR_ARG, "%s: give both terminators or neither", who);
    if (kind == 0 && (coef_a == nullptr) != (coef_b == nullptr)) return fail(h, RSREC_ERR_ARG, "%s: give both a_b and b_sqrt or neither", who);
    if (kind == 0 && !a_inf && lld < 2) return fail(h, RSREC_ERR_ARG, "%s: the device terminator needs lld >= 2", who);
    c.who = who; c.kind = kind; c.npairs = npairs; c.lld = lld; c.nen = nen; c.per = per;
    c.a_inf = a_inf; c.b_inf = b_inf; c.coef_a = coef_a; c.coef_b = coef_b;
    c.row_doubles = row_doubles; c.fixed_out = fixed_out; c.chunk_out = chunk_out;
    const int nchains = per * npairs;
    c.resident = coef_a == nullptr;
    int nsame = 0;
    for (int p = 0; p < npairs; ++p) nsame += (per == 4 && same[p] != 0);
    // first chain of every pair: slot order (4 per pair), or -- resident chains of a seeded call that skipped the repeats of i == j
    // pairs (recur_b_ij, recursion.f90:1705) -- 1 chain for such a pair
    c.compact = c.resident && nsame > 0 && h->res_n == nchains - 3 * nsame;
    if (c.resident && (h->res_kind != (kind == 0 ? 1 : 2) || (h->res_n != nchains && !c.compact) || h->res_lld != lld))
        return fail(h, RSREC_ERR_ARG, "%s: no %s chains of %d %s at lld = %d resident (call the %s first)", who,
                    kind == 0 ? "block-Lanczos" : "Chebyshev", npairs, per == 4 ? "pairs" : "sites", lld, per == 4 ? "seeded recursion" : "on-site recursion");
    if (c.resident && per == 1 && h->res_seeded)     // 4 * npairs seeded chains are not nsites on-site chains, whatever their count
        return fail(h, RSREC_ERR_ARG, "%s: the resident chains are those of a seeded pair recursion, not on-site chains (call the on-site recursion first)", who);
    if (c.compact && a_inf)        // terminators come in slot order (4 per pair); the compacted chains have no slot for the skipped repeats
        return fail(h, RSREC_ERR_ARG, "%s: resident chains with skipped i == j repeats take no caller terminators (pass NULL)", who);
    c.nm = 2 * lld + 2;
    if (kind == 1 && c.nm > (int)((64 * 1024) / sizeof(double2))) return fail(h, RSREC_ERR_ARG, "%s: lld = %d too deep for the Chebyshev phase table", who, lld);
    c.cbase.assign(npairs + 1, 0);
    for (int p = 0; p < npairs; ++p) c.cbase[p + 1] = c.cbase[p] + ((c.compact && same[p]) ? 1 : per);
    HIPCK(h, hipSetDevice(h->device));
    const int nm = c.nm;
    c.cel = kind == 0 ? (size_t)lld * BLK : (size_t)nm * BLK;
    const size_t cel = c.cel;
    const size_t rbytes = row_doubles * sizeof(double);                                    // rows of one pair
    const size_t cbytes = (size_t)per * cel * sizeof(double2) * (kind == 0 ? 2 : 1);      // coefficients of one pair
    // pairs per chunk: the row scratch <= 256 MiB and the staged coefficients <= 512 MiB, whatever npairs
    c.P = (int)std::max<size_t>(1, std::min<size_t>((size_t)npairs, std::min(((size_t)256 << 20) / rbytes, ((size_t)512 << 20) / cbytes)));
    // RSREC_PAIR_CHUNK (environment, for tests): an upper limit on the pairs per chunk, so that small calls run the multi-chunk loop
    if (const char* cap = getenv("RSREC_PAIR_CHUNK")) c.P = std::max(1, std::min(c.P, atoi(cap)));
    c.P = std::max(group, c.P - c.P % group);                                              // whole groups of pairs (the trios of rsrec_spin_lattice)
    const size_t P = (size_t)c.P;
    release_kubo_buffers(h, true, true);
    // every region starts at an even double: the kernels read complex numbers as double2
    const size_t off_fixed = even(nen), off_same = off_fixed + even(fixed_in), off_cb = off_same + even((npairs + 1) / 2 + 1);
    c.off_ab = off_cb + even((npairs + 2) / 2 + 1);
    const size_t Q = (size_t)per * P;                                                    // chain slots per chunk
    c.off_bs = c.off_ab + Q * cel * 2;
    c.off_ai = c.off_bs + (kind == 0 ? Q * cel * 2 : 0);
    c.off_bi = c.off_ai + even(std::max<size_t>(Q * BLK, nm));
    const size_t off_chunk = c.off_bi + Q * BLK;
    HIPCK(h, h->d_green_in.reserve((off_chunk + P * chunk_in) * sizeof(double)));
    const size_t off_fo = P * row_doubles, off_co = off_fo + fixed_out;
    HIPCK(h, h->d_green_out.reserve((off_co + P * chunk_out) * sizeof(double)));
    if (c.resident && kind == 0) HIPCK(h, h->d_bsqrt.reserve(Q * cel * sizeof(double2)));      // resident_block_prologue's, for the largest chunk
    HIPCK(h, h->d_status.reserve(64));
    HIPCK(h, hipMemsetAsync(h->d_status.p, 0, 64, h->stream));
    c.din = h->d_green_in.as<double>();
    c.d_ene = c.din;
    c.d_fixed_in = c.din + off_fixed;
    c.d_same = reinterpret_cast<int*>(c.din + off_same);
    c.d_cb = reinterpret_cast<int*>(c.din + off_cb);
    c.d_chunk_in = c.din + off_chunk;
    c.d_rows = h->d_green_out.as<double>();
    c.d_fixed_out = c.d_rows + off_fo;
    c.d_chunk_out = c.d_rows + off_co;
    XFER(xfer_h2d(h, c.d_ene, ene, (size_t)nen * sizeof(double)));
    XFER(xfer_h2d(h, c.d_same, same, (size_t)npairs * sizeof(int32_t)));
    XFER(xfer_h2d(h, c.d_cb, c.cbase.data(), (size_t)(npairs + 1) * sizeof(int)));
    chebyshev_green_scaling(energy_min, energy_max, c.ca, c.cb);
    if (kind == 1) {
        const std::vector<double> kern = chebyshev_green_kernel(nm);
        XFER(xfer_h2d(h, c.din + c.off_ai, kern.data(), (size_t)nm * sizeof(double)));      // (the terminator slot is unused by kind 1)
    }
    return RSREC_OK;
}

// Coefficients and terminators of the pairs p0 .. p0 + P - 1 (resident: read in place, behind resident_block_prologue; caller
// arrays: staged, or read in place when they are device memory; terminators from the device unless given)
int pair_call_chunk(rsrec_t* h, const PairCall& c, int p0, PairChunk& k) {
    const size_t cel = c.cel;
    k.np = std::min(c.P, c.npairs - p0);
    const size_t c0 = (size_t)c.cbase[p0], nc = (size_t)(c.cbase[p0 + k.np] - c.cbase[p0]);     // chains of the chunk
    k.c0 = (int)c0;
    k.sb = nullptr; k.tb = nullptr;
    double* const d_ai = c.din + c.off_ai;
    double* const d_bi = c.din + c.off_bi;
    const double* sa = nullptr;
    if (c.resident) sa = reinterpret_cast<const double*>((c.kind == 0 ? h->d_coefA.as<double2>() : h->d_mu.as<double2>()) + c0 * cel);
    else XFER(xc_fetch(h, c.coef_a + c0 * cel * 2, c.din + c.off_ab, nc * cel * 2, &sa));
    k.sa = reinterpret_cast<const double2*>(sa);
    k.ta = d_ai;
    if (c.kind == 1) return RSREC_OK;
    k.tb = d_bi;
    if (c.resident) {
        XFER(resident_block_prologue(h, c0, nc, c.lld, c.a_inf ? nullptr : d_ai, d_bi));
        k.sb = h->d_bsqrt.as<double2>();
    } else {
        const double* sb = nullptr;
        XFER(xc_fetch(h, c.coef_b + c0 * cel * 2, c.din + c.off_bs, nc * cel * 2, &sb));
        k.sb = reinterpret_cast<const double2*>(sb);
        if (!c.a_inf) XFER(launch_terminator(h, (int)nc, c.lld, k.sa, k.sb, d_ai, d_bi));
    }
    if (c.a_inf) {
        XFER(xc_fetch(h, c.a_inf + c0 * BLK, d_ai, nc * BLK, &k.ta));
        XFER(xc_fetch(h, c.b_inf + c0 * BLK, d_bi, nc * BLK, &k.tb));
    }
    return RSREC_OK;
}

// an image of such a call for the caller: n doubles at `off` of the call's own outputs
struct PairImage { double* dst; size_t off, n; };

// The call that pair_call_begin set up: its own outputs zeroed and, where `fermi` is given, the Fermi weights in the first nen doubles
// of its own inputs; then chunk by chunk the coefficients, stage(p0, k) (the fetch of the chunk's own inputs), kernel(p0, k) and
// reduce(p0, k) (one launch each, timed together as the kernel stage) and the chunk's outputs and rows to `chunk_out` and `rows`
// where given; then the images, the status word, the stream and the timing (total; hop = rest = the kernel stages of the chunks).
template <class Stage, class Kernel, class Reduce>
int pair_call_run(rsrec_t* h, const PairCall& c, const double* fermi, double* chunk_out, double* rows, std::initializer_list<PairImage> images,
                  Stage stage, Kernel kernel, Reduce reduce) {
    reset_timing(h);
    hipEvent_t e0 = next_event(h);
    // (a value that runs across the chunks, rsrec_damping's total, lives in these outputs: this one memset is what starts it at zero)
    HIPCK(h, hipMemsetAsync(c.d_fixed_out, 0, c.fixed_out * sizeof(double), h->stream));
    if (fermi) k_exchange_fermi<<<(c.nen + 255) / 256, 256, 0, h->stream>>>(c.nen, c.d_ene, *fermi, c.d_fixed_in);
    std::vector<std::pair<hipEvent_t, hipEvent_t>> kev;
    for (int p0 = 0; p0 < c.npairs; p0 += c.P) {
        PairChunk k;
        XFER(pair_call_chunk(h, c, p0, k));
        XFER(stage(p0, k));
        std::pair<hipEvent_t, hipEvent_t> ev;
        ev.first = next_event(h);
        kernel(p0, k);
        HIPCK(h, hipGetLastError());
        reduce(p0, k);
        HIPCK(h, hipGetLastError());
        ev.second = next_event(h);
        kev.push_back(ev);
        if (chunk_out) XFER(xc_deliver(h, chunk_out + (size_t)p0 * c.chunk_out, c.d_chunk_out, (size_t)k.np * c.chunk_out));
        if (rows) XFER(xc_deliver(h, rows + (size_t)p0 * c.row_doubles, c.d_rows, (size_t)k.np * c.row_doubles));
        if (p0 + c.P < c.npairs) HIPCK(h, hipStreamSynchronize(h->stream));       // the chunk's staging buffers are reused
    }
    for (const PairImage& im : images) XFER(xc_deliver(h, im.dst, c.d_fixed_out + im.off, im.n));
    hipEvent_t e1 = next_event(h);
    const int rc = finish_status(h);
    h->t_total_ms = ev_ms(e0, e1);
    h->t_rest_ms = 0.0;
    for (auto& pr : kev) h->t_rest_ms += ev_ms(pr.first, pr.second);
    h->t_hop_ms = h->t_rest_ms;
    return rc;
}

// (a call whose chunks have no inputs of their own)
int no_stage(int, const PairChunk&) { return RSREC_OK; }

// simpson_f's mesh, for the calls that integrate over the energies
int check_simpson_mesh(rsrec_t* h, const char* who, int nen, int nv1) {
    if (nen < nv1 + 9) return fail(h, RSREC_ERR_ARG, "%s: nen = %d < nv1 + 9 = %d (simpson_f integrates to nv1 + 10)", who, nen, nv1 + 9);
    return RSREC_OK;
}

// the Chebyshev kernels that keep `shared` bytes of dressed blocks in LDS beside the phase table (those of a pair, or of a trio)
int check_cheb_lds(rsrec_t* h, const char* who, int kind, int lld, size_t shared, const char* whose) {
    if (kind == 1 && (size_t)(2 * lld + 2) * sizeof(double2) + sizeof(XcChebLds) + shared > (size_t)64 * 1024)
        return fail(h, RSREC_ERR_ARG, "%s: lld = %d too deep for the Chebyshev phase table beside the %s's blocks", who, lld, whose);
    return RSREC_OK;
}

}  // namespace

// green%calculate_intersite_gf / _twoindex + exchange%calculate_exchange / _twoindex (integrands and integrals) for the pairs of one rank.
extern "C" int rsrec_exchange(rsrec_t* h, int kind, int npairs, const int32_t* same, int lld, int nen, const double* ene, int nv1, double fermi,
                              int sym_term, double energy_min, double energy_max, const double* a_inf, const double* b_inf, const double* coef_a,
                              const double* coef_b, const double* dpar, int pair_offset, int npairs_total, double* xc, double* so, double* fo,
                              double* parts, double* jcum, double* integrand) {
    if (!h) return RSREC_ERR_ARG;
    if (npairs < 1 || lld < 1 || nv1 < 1 || !same || !ene || !dpar || !xc || !so || !fo || !parts || pair_offset < 0 || npairs_total < pair_offset + npairs)
        return fail(h, RSREC_ERR_ARG, "rsrec_exchange: bad argument");
    XFER(check_simpson_mesh(h, "rsrec_exchange", nen, nv1));
    const size_t nt = (size_t)npairs_total, nimg = (size_t)XC_NOUT * nt;
    PairCall c;
    // own inputs: fermi weights | dpar;  own outputs: the images (xc, so, fo, parts) and jcum of the chunk
    XFER(pair_call_begin(h, c, "rsrec_exchange", kind, npairs, same, lld, nen, ene, energy_min, energy_max, a_inf, b_inf, coef_a, coef_b,
                         (size_t)nen * XC_NINT, (size_t)nen + (size_t)24 * npairs, 0, nimg, (size_t)nen));
    double* d_fw = c.d_fixed_in;
    double* d_dpar = d_fw + nen;
    double* d_img = c.d_fixed_out;
    XFER(xfer_h2d(h, d_dpar, dpar, (size_t)24 * npairs * sizeof(double)));
    return pair_call_run(h, c, &fermi, jcum, integrand, {{xc, 0, 13 * nt}, {so, 13 * nt, 13 * nt}, {fo, 26 * nt, 13 * nt}, {parts, 39 * nt, 28 * nt}}, no_stage,
        [&](int p0, const PairChunk& k) {
            if (kind == 0)
                k_exchange_block<<<dim3(nen, k.np), 256, 0, h->stream>>>(lld, nen, c.d_ene, sym_term, k.ta, k.tb, k.sa, k.sb, c.d_same + p0, c.d_cb + p0, k.c0,
                                                                      d_dpar + (size_t)24 * p0, c.d_rows);
            else
                k_exchange_cheb<<<dim3(nen, k.np), 256, (size_t)c.nm * sizeof(double2), h->stream>>>(c.nm, nen, c.d_ene, c.ca, c.cb, k.ta, k.sa, c.d_same + p0,
                                                                                                   c.d_cb + p0, k.c0, d_dpar + (size_t)24 * p0, c.d_rows);
        },
        [&](int p0, const PairChunk& k) {
            k_exchange_integrate<<<k.np, 128, 0, h->stream>>>(nen, nv1, c.d_ene, d_fw, c.d_rows, pair_offset + p0, d_img, d_img + 13 * nt, d_img + 26 * nt,
                                                              d_img + 39 * nt, jcum ? c.d_chunk_out : nullptr, 0);
        });
}

// exchange%calculate_gilbert_damping (exchange.f90:674-694) for the pairs of one rank: the nine traces Tr(T_i^k Aij (T_j^l)^H Aji) per
// energy, without gij / gji or the reference's temporaries.
extern "C" int rsrec_damping(rsrec_t* h, int kind, int npairs, const int32_t* same, int lld, int nen, const double* ene, int ief, int sym_term,
                             double energy_min, double energy_max, const double* a_inf, const double* b_inf, const double* coef_a, const double* coef_b,
                             const double* tmat, int pair_offset, int npairs_total, double* at_ef, double* total, double* rows) {
    if (!h) return RSREC_ERR_ARG;
    if (npairs < 1 || lld < 1 || nen < 1 || !same || !ene || !at_ef || !total || pair_offset < 0 || npairs_total < pair_offset + npairs)
        return fail(h, RSREC_ERR_ARG, "rsrec_damping: bad argument");
    if (!tmat) return fail(h, RSREC_ERR_ARG, "rsrec_damping: no torque matrices (tmat is NULL)");
    if (ief < 1 || ief > nen) return fail(h, RSREC_ERR_ARG, "rsrec_damping: ief = %d outside 1..%d", ief, nen);
    const size_t nimg = (size_t)DP_NROW * npairs_total, ntot = (size_t)9 * nen;
    PairCall c;
    // own chunk inputs: tmat of the chunk's pairs;  own outputs: the at_ef image | total, k_damping_reduce adding to it chunk after chunk
    XFER(pair_call_begin(h, c, "rsrec_damping", kind, npairs, same, lld, nen, ene, energy_min, energy_max, a_inf, b_inf, coef_a, coef_b,
                         (size_t)nen * DP_NROW, 0, (size_t)2 * DP_TMAT, nimg + ntot, 0));
    double* d_img = c.d_fixed_out;
    const double* tm = nullptr;
    return pair_call_run(h, c, nullptr, nullptr, rows, {{at_ef, 0, nimg}, {total, nimg, ntot}},
        [&](int p0, const PairChunk& k) { return xc_fetch(h, tmat + (size_t)p0 * 2 * DP_TMAT, c.d_chunk_in, (size_t)k.np * 2 * DP_TMAT, &tm); },
        [&](int p0, const PairChunk& k) {
            if (kind == 0)
                k_damping_block<<<dim3(nen, k.np), 256, 0, h->stream>>>(lld, nen, c.d_ene, sym_term, k.ta, k.tb, k.sa, k.sb, c.d_same + p0, c.d_cb + p0, k.c0,
                                                                     reinterpret_cast<const double2*>(tm), c.d_rows);
            else
                k_damping_cheb<<<dim3(nen, k.np), 256, (size_t)c.nm * sizeof(double2), h->stream>>>(c.nm, nen, c.d_ene, c.ca, c.cb, k.ta, k.sa, c.d_same + p0,
                                                                                                  c.d_cb + p0, k.c0, reinterpret_cast<const double2*>(tm), c.d_rows);
        },
        [&](int p0, const PairChunk& k) {
            k_damping_reduce<<<(unsigned)((ntot + (size_t)DP_NROW * k.np + 255) / 256), 256, 0, h->stream>>>(nen, k.np, ief - 1, c.d_rows, pair_offset + p0, d_img,
                                                                                                             d_img + nimg);
        });
}

// exchange%calculate_jij_auxgreen (exchange.f90:171-335) for the pairs of one rank: the 9 tensor components (or J00) per energy from the
// dressed up-up and down-down blocks of gij / gji (kernels_auxgreen.hpp), and their Fermi-weighted Simpson integrals, unscaled.
extern "C" int rsrec_exchange_aux(rsrec_t* h, int kind, int npairs, const int32_t* same, int lld, int nen, const double* ene, int nv1, double fermi,
                                  int sym_term, double energy_min, double energy_max, const double* a_inf, const double* b_inf, const double* coef_a,
                                  const double* coef_b, const double* apar, int pair_offset, int npairs_total, double* jaux, double* rows) {
    if (!h) return RSREC_ERR_ARG;
    if (npairs < 1 || lld < 1 || nv1 < 1 || !same || !ene || pair_offset < 0 || npairs_total < pair_offset + npairs)
        return fail(h, RSREC_ERR_ARG, "rsrec_exchange_aux: bad argument");
    if (!apar) return fail(h, RSREC_ERR_ARG, "rsrec_exchange_aux: no potential parameters (apar is NULL)");
    if (!jaux) return fail(h, RSREC_ERR_ARG, "rsrec_exchange_aux: no output (jaux is NULL)");
    XFER(check_cheb_lds(h, "rsrec_exchange_aux", kind, lld, sizeof(AuxShared), "pair"));
    XFER(check_simpson_mesh(h, "rsrec_exchange_aux", nen, nv1));
    const size_t nimg = (size_t)AX_NROW * npairs_total;
    PairCall c;
    // own inputs: fermi weights;  own chunk inputs: apar of the chunk's pairs;  own output: the jaux image
    XFER(pair_call_begin(h, c, "rsrec_exchange_aux", kind, npairs, same, lld, nen, ene, energy_min, energy_max, a_inf, b_inf, coef_a, coef_b,
                         (size_t)nen * AX_NROW, (size_t)nen, (size_t)2 * AX_APAR, nimg, 0));
    const double* ap = nullptr;
    return pair_call_run(h, c, &fermi, nullptr, rows, {{jaux, 0, nimg}},
        [&](int p0, const PairChunk& k) { return xc_fetch(h, apar + (size_t)p0 * 2 * AX_APAR, c.d_chunk_in, (size_t)k.np * 2 * AX_APAR, &ap); },
        [&](int p0, const PairChunk& k) {
            if (kind == 0)
                k_aux_block<<<dim3(nen, k.np), 256, 0, h->stream>>>(lld, nen, c.d_ene, sym_term, k.ta, k.tb, k.sa, k.sb, c.d_same + p0, c.d_cb + p0, k.c0, ap,
                                                                 c.d_rows);
            else
                k_aux_cheb<<<dim3(nen, k.np), 256, (size_t)c.nm * sizeof(double2), h->stream>>>(c.nm, nen, c.d_ene, c.ca, c.cb, k.ta, k.sa, c.d_same + p0,
                                                                                              c.d_cb + p0, k.c0, ap, c.d_rows);
        },
        [&](int p0, const PairChunk& k) {
            k_rows_integrate<<<k.np, 64, 0, h->stream>>>(nen, nv1, AX_NROW, c.d_ene, c.d_fixed_in, c.d_rows, pair_offset + p0, c.d_fixed_out);
        });
}

// exchange%calculate_jijk (exchange.f90:338-601) for the trios of one rank.  The pairs of trio t are 3 t .. 3 t + 2 = (i,j), (i,k), (j,k)
// (lattice.f90:644-651); one workgroup per (trio, energy) runs their Green stages one after another and keeps the dressed blocks in LDS.
extern "C" int rsrec_spin_lattice(rsrec_t* h, int kind, int npairs, const int32_t* same, int lld, int nen, const double* ene, int nv1, double fermi,
                                  int sym_term, double energy_min, double energy_max, const double* a_inf, const double* b_inf, const double* coef_a,
                                  const double* coef_b, const double* apar, const double* dmat, int trio_offset, int ntrios_total, double* jijk,
                                  double* rows) {
    if (!h) return RSREC_ERR_ARG;
    if (npairs < 1 || lld < 1 || nv1 < 1 || !same || !ene || trio_offset < 0) return fail(h, RSREC_ERR_ARG, "rsrec_spin_lattice: bad argument");
    if (npairs % 3) return fail(h, RSREC_ERR_ARG, "rsrec_spin_lattice: npairs = %d is not a multiple of 3 (a trio is the pairs (i,j), (i,k), (j,k))", npairs);
    if (ntrios_total < trio_offset + npairs / 3) return fail(h, RSREC_ERR_ARG, "rsrec_spin_lattice: bad argument");
    if (!apar) return fail(h, RSREC_ERR_ARG, "rsrec_spin_lattice: no potential parameters (apar is NULL)");
    if (!dmat) return fail(h, RSREC_ERR_ARG, "rsrec_spin_lattice: no displacement matrices (dmat is NULL)");
    if (!jijk) return fail(h, RSREC_ERR_ARG, "rsrec_spin_lattice: no output (jijk is NULL)");
    XFER(check_simpson_mesh(h, "rsrec_spin_lattice", nen, nv1));
    XFER(check_cheb_lds(h, "rsrec_spin_lattice", kind, lld, sizeof(JkShared), "trio"));
    const size_t nimg = (size_t)AX_NROW * ntrios_total;
    constexpr size_t TRIO_IN = (size_t)3 * JK_APAR + 2 * 81;                                   // apar | dmat of one trio
    static_assert(TRIO_IN % 3 == 0 && (3 * JK_APAR) % 2 == 0 && AX_NROW % 3 == 0, "a trio's inputs and rows split over its pairs; dmat is read as double2");
    PairCall c;
    // chunks of whole trios.  Per pair: a third of a trio's rows and inputs.  Own inputs: fermi weights;  own output: the jijk image
    XFER(pair_call_begin(h, c, "rsrec_spin_lattice", kind, npairs, same, lld, nen, ene, energy_min, energy_max, a_inf, b_inf, coef_a, coef_b,
                         (size_t)nen * AX_NROW / 3, (size_t)nen, TRIO_IN / 3, nimg, 0, 4, 3));
    double* d_ap = c.d_chunk_in;
    double* d_dm = d_ap + (size_t)(c.P / 3) * 3 * JK_APAR;
    const double *ap = nullptr, *dm = nullptr;
    return pair_call_run(h, c, &fermi, nullptr, rows, {{jijk, 0, nimg}},
        [&](int p0, const PairChunk& k) {
            const size_t t0 = p0 / 3, nt = k.np / 3;
            XFER(xc_fetch(h, apar + t0 * 3 * JK_APAR, d_ap, nt * 3 * JK_APAR, &ap));
            return xc_fetch(h, dmat + t0 * 2 * 81, d_dm, nt * 2 * 81, &dm);
        },
        [&](int p0, const PairChunk& k) {
            if (kind == 0)
                k_jijk_block<<<dim3(nen, k.np / 3), 256, 0, h->stream>>>(lld, nen, c.d_ene, sym_term, k.ta, k.tb, k.sa, k.sb, c.d_same + p0, c.d_cb + p0, k.c0, ap,
                                                                      reinterpret_cast<const double2*>(dm), c.d_rows);
            else
                k_jijk_cheb<<<dim3(nen, k.np / 3), 256, (size_t)c.nm * sizeof(double2), h->stream>>>(c.nm, nen, c.d_ene, c.ca, c.cb, k.ta, k.sa, c.d_same + p0,
                                                                                                   c.d_cb + p0, k.c0, ap, reinterpret_cast<const double2*>(dm), c.d_rows);
        },
        [&](int p0, const PairChunk& k) {
            k_rows_integrate<<<k.np / 3, 64, 0, h->stream>>>(nen, nv1, AX_NROW, c.d_ene, c.d_fixed_in, c.d_rows, trio_offset + p0 / 3, c.d_fixed_out);
        });
}

namespace {

// eta_k = (1 - x_k) / x_k of the contour points, as the reference forms it (green.f90:507-508, bands.f90:562-563): eta = cmplx(0.0_rp, res)
// has no KIND, so it is default (single-precision) complex and res passes through float before it is added to the energy
int contour_eta(rsrec_t* h, const char* who, int npts, const double* x, std::vector<double>& eta) {
    eta.resize(npts);
    for (int k = 0; k < npts; ++k) {
        if (!(x[k] > 0.0)) return fail(h, RSREC_ERR_ARG, "%s: x(%d) = %g is not a node on (0, 1]", who, k + 1, x[k]);
        eta[k] = (double)(float)((1 - x[k]) / x[k]);
    }
    return RSREC_OK;
}

}  // namespace

// green%calculate_intersite_gf_eta + exchange%calculate_exchange_gauss_legendre for the pairs of one rank (kernels_contour.hpp).
extern "C" int rsrec_exchange_contour(rsrec_t* h, int kind, int npairs, const int32_t* same, int lld, int npts, const double* x, const double* w, double e0,
                                      int sym_term, double energy_min, double energy_max, const double* a_inf, const double* b_inf, const double* coef_a,
                                      const double* coef_b, const double* dmat, int pair_offset, int npairs_total, double* xc, double* rows) {
    if (!h) return RSREC_ERR_ARG;
    if (npts < 1 || npairs < 1 || lld < 1 || !same || !x || !w || !xc || pair_offset < 0 || npairs_total < pair_offset + npairs)
        return fail(h, RSREC_ERR_ARG, "rsrec_exchange_contour: bad argument");
    if (!dmat) return fail(h, RSREC_ERR_ARG, "rsrec_exchange_contour: no dmat (NULL)");
    if (is_device_ptr(x) || is_device_ptr(w)) return fail(h, RSREC_ERR_ARG, "rsrec_exchange_contour: x and w are host arrays");
    std::vector<double> eta;
    XFER(contour_eta(h, "rsrec_exchange_contour", npts, x, eta));
    const size_t nimg = (size_t)CT_NROW * npairs_total;
    PairCall c;
    // the "energies" of the call are the points' eta;  own inputs: x | w;  own chunk inputs: dmat of the chunk's pairs;  own output: the xc image
    XFER(pair_call_begin(h, c, "rsrec_exchange_contour", kind, npairs, same, lld, npts, eta.data(), energy_min, energy_max, a_inf, b_inf, coef_a, coef_b,
                         (size_t)npts * CT_NROW, (size_t)2 * npts, (size_t)CT_DMAT, nimg, 0));
    double* d_x = c.d_fixed_in;
    double* d_w = d_x + npts;
    XFER(xfer_h2d(h, d_x, x, (size_t)npts * sizeof(double)));
    XFER(xfer_h2d(h, d_w, w, (size_t)npts * sizeof(double)));
    const double* dm = nullptr;
    return pair_call_run(h, c, nullptr, nullptr, rows, {{xc, 0, nimg}},           // (the terminators: once per chain, not once per point)
        [&](int p0, const PairChunk& k) { return xc_fetch(h, dmat + (size_t)p0 * CT_DMAT, c.d_chunk_in, (size_t)k.np * CT_DMAT, &dm); },
        [&](int p0, const PairChunk& k) {
            if (kind == 0)
                k_contour_xc_block<<<dim3(npts, k.np), 256, 0, h->stream>>>(lld, npts, e0, c.d_ene, d_x, d_w, sym_term, k.ta, k.tb, k.sa, k.sb, c.d_same + p0,
                                                                         c.d_cb + p0, k.c0, dm, c.d_rows);
            else
                k_contour_xc_cheb<<<dim3(npts, k.np), 256, (size_t)c.nm * sizeof(double2), h->stream>>>(c.nm, npts, e0, c.d_ene, d_x, d_w, c.ca, c.cb, k.ta, k.sa,
                                                                                                      c.d_same + p0, c.d_cb + p0, k.c0, dm, c.d_rows);
        },
        [&](int p0, const PairChunk& k) {
            k_contour_xc_sum<<<(k.np * CT_NROW + 255) / 256, 256, 0, h->stream>>>(npts, k.np, c.d_rows, pair_offset + p0, c.d_fixed_out);
        });
}

// The occupations of bands%calculate_moments_gauss_legendre / calculate_occupation_gauss_legendre for the on-site chains of one rank.
extern "C" int rsrec_contour_occupation(rsrec_t* h, int kind, int nsites, int lld, int npts, const double* x, const double* w, double e0, int sym_term,
                                        double energy_min, double energy_max, const double* a_inf, const double* b_inf, const double* coef_a,
                                        const double* coef_b, int site_offset, int nsites_total, double* occ, double* gdiag) {
    if (!h) return RSREC_ERR_ARG;
    if (npts < 1 || nsites < 1 || lld < 1 || !x || !w || !occ || site_offset < 0 || nsites_total < site_offset + nsites)
        return fail(h, RSREC_ERR_ARG, "rsrec_contour_occupation: bad argument");
    if (is_device_ptr(x) || is_device_ptr(w)) return fail(h, RSREC_ERR_ARG, "rsrec_contour_occupation: x and w are host arrays");
    std::vector<double> eta;
    XFER(contour_eta(h, "rsrec_contour_occupation", npts, x, eta));
    const size_t nimg = (size_t)NB * nsites_total;
    const std::vector<int32_t> same(nsites, 0);
    PairCall c;
    // one chain per site;  own inputs: x | w;  own output: the occ image;  the rows of a chunk: the diagonal of g at every point
    XFER(pair_call_begin(h, c, "rsrec_contour_occupation", kind, nsites, same.data(), lld, npts, eta.data(), energy_min, energy_max, a_inf, b_inf, coef_a,
                         coef_b, (size_t)npts * NB * 2, (size_t)2 * npts, 0, nimg, 0, 1));
    double* d_x = c.d_fixed_in;
    double* d_w = d_x + npts;
    double2* d_gd = reinterpret_cast<double2*>(c.d_rows);
    XFER(xfer_h2d(h, d_x, x, (size_t)npts * sizeof(double)));
    XFER(xfer_h2d(h, d_w, w, (size_t)npts * sizeof(double)));
    return pair_call_run(h, c, nullptr, nullptr, gdiag, {{occ, 0, nimg}}, no_stage,
        [&](int, const PairChunk& k) {
            if (kind == 0)
                k_contour_occ_block<<<dim3((npts + GREEN_WAVES - 1) / GREEN_WAVES, k.np), GREEN_WAVES * 64, 0, h->stream>>>(lld, npts, e0, c.d_ene, sym_term, k.ta,
                                                                                                                         k.tb, k.sa, k.sb, d_gd);
            else
                k_contour_occ_cheb<<<dim3(npts, k.np), 64, (size_t)c.nm * sizeof(double2), h->stream>>>(c.nm, npts, e0, c.d_ene, c.ca, c.cb, k.ta, k.sa, d_gd);
        },
        [&](int s0, const PairChunk& k) {
            k_contour_occ_sum<<<(k.np * NB + 255) / 256, 256, 0, h->stream>>>(npts, k.np, d_x, d_w, d_gd, site_offset + s0, c.d_fixed_out);
        });
}

namespace {

// behind a batch's staged seed coefficients, one mu_1 scale per chain: sum over its seed atoms of |final coefficient|^2 (later seeds overwrite earlier ones on the same atom)
void cheb_mu1_scales(int nb, int nseed, const std::vector<int>& seeds0, std::vector<double>& coef) {
    coef.resize((size_t)nb * nseed * 2 + nb);
    for (int c = 0; c < nb; ++c) {
        double m0 = 0.0;
        for (int k = 0; k < nseed; ++k) {
            bool overwritten = false;
            for (int k2 = k + 1; k2 < nseed; ++k2) overwritten |= seeds0[(size_t)c * nseed + k2] == seeds0[(size_t)c * nseed + k];
            const size_t q = (size_t)c * nseed + k;
            if (!overwritten) m0 += coef[2 * q] * coef[2 * q] + coef[2 * q + 1] * coef[2 * q + 1];
        }
        coef[(size_t)nb * nseed * 2 + c] = m0;
    }
}

template <bool MFMA>
int run_chebyshev(rsrec_t* h, int nsites, int nseed, const int32_t* seed_atoms, const double* seed_coef, int lld, double a, double b, double* mu_n) {
    const int kk = h->kk;
    const bool hoh = h->hoh != 0;
    const int napply = lld + 1;                                  // first moment + lld steps
    const int nmom = 2 * lld + 2;
    RecursionCall RC = recursion_call(h, MFMA, nsites, nseed, napply);
    const int ci = RC.ci;
    const size_t mstride = (size_t)nmom * BLK;
    // the moments of ALL chains of the call stay on the device (rsrec_pack_moments): reserved BEFORE the batch is planned from the free
    // memory, so a call over many sites (nrec ~ kk) sizes its vectors around them instead of failing behind them
    drop_resident(h);
    HIPCK(h, h->d_mu.reserve((size_t)nsites * nmom * BLK * sizeof(double2)));
    // k_spmm5 forms the new vector in its epilogue (cur = (H old - b old)/a [* 2 - spare]; the default of the matrix-core set); k_mfma_cheb then
    // only sums the Grams and H psi is never held: vector 3 is neither allocated nor cleared
    const bool fused = ci && h->opt_cheb_fused;
    XFER(recursion_begin(h, RC, MFMA ? (hoh ? 5 : 4) : (hoh ? 4 : 3), fused ? 3 : -1, nseed + 1));
    const int nblk = RC.nblk;
    SideReduce SR{RC.side};               // moment reduction of level t under the SpMM of level t + 1 (it feeds nothing on the device)
    for (int c0 = 0; c0 < nsites; c0 += RC.B) {
        const int nb = std::min(RC.B, nsites - c0);
        double2* mu = h->d_mu.as<double2>() + (size_t)c0 * mstride;       // this batch's slice of the resident moments
        RecursionBatch bt;
        XFER(recursion_batch(h, RC, seed_atoms, seed_coef, c0, nb, bt, cheb_mu1_scales));
        const ChainView& CVp = bt.CVp;
        XFER(clear_vectors(h, RC, nb));
        HIPCK(h, hipMemsetAsync(mu, 0, (size_t)nb * mstride * sizeof(double2), h->stream));
        ChainChebyshev S(h, RC, a, b);
        seed_chains(h, RC, nb, S.cur);
        k_set_identity<<<nb, 256, 0, h->stream>>>(mu, mstride, h->d_seedcoef.as<double>() + (size_t)nb * nseed * 2);   // mu_1 (cheb_0th_mom :2157)
        for (int t = 1; t <= napply; ++t) {      // t = 1: first moment; t >= 2: recursion step ll = t-1
            const bool first = (t == 1);
            XFER(S.step(h, RC, bt, t, MFMA && !fused));        // unfused: H old is in S.tmp and k_mfma_cheb forms S.cur
            if (MFMA) {
                const dim3 gl = level_grid(h, bt.grid_mf, S.level);
                double* gp = h->d_partial.as<double>();
                XFER(side_reduce_wait(h, SR));                    // gp is free again
                if (fused) {
                    if (first) k_mfma_cheb<true, true><<<gl, MF_WAVES * 64, 0, h->stream>>>(CVp, S.level, kk, nullptr, S.old, nullptr, S.cur, a, b, gp);
                    else k_mfma_cheb<false, true><<<gl, MF_WAVES * 64, 0, h->stream>>>(CVp, S.level, kk, nullptr, S.old, nullptr, S.cur, a, b, gp);
                } else if (first) k_mfma_cheb<true><<<gl, MF_WAVES * 64, 0, h->stream>>>(CVp, S.level, kk, S.tmp, S.old, nullptr, S.cur, a, b, gp);
                else k_mfma_cheb<false><<<gl, MF_WAVES * 64, 0, h->stream>>>(CVp, S.level, kk, S.tmp, S.old, S.spare, S.cur, a, b, gp);
                hipStream_t rs; XFER(side_reduce_begin(h, SR, rs));
                int n2 = gl.x; const double* gp2 = presum(h, gp, nb, n2, 2 * 1296, rs, SR.side ? 1 : 0);
                k_reduce_cheb_mf<<<nb, 1024, 0, rs>>>(gp2, n2, first ? 1 : 0, t - 1, mu, mstride, h->d_status.as<int>(), nseed > 1 ? 1 : 0, ci);
                XFER(side_reduce_end(h, SR));
                continue;
            }
            k_reduce_cheb<<<nb, 1024, 0, h->stream>>>(h->d_partial.as<double2>(), nblk, first ? 1 : 0, t - 1, mu, mstride, h->d_status.as<int>(), nseed > 1 ? 1 : 0);
        }
        HIPCK(h, hipGetLastError());
        XFER(side_reduce_wait(h, SR));
        XFER(xfer_d2h(h, mu_n + (size_t)c0 * mstride * 2, mu, (size_t)nb * mstride * sizeof(double2)));
        HIPCK(h, hipStreamSynchronize(h->stream));
    }
    return recursion_end(h, RC, 2, lld, seed_coef != nullptr);
}

}  // namespace

extern "C" int rsrec_chebyshev_seeded(rsrec_t* h, int nchains, int nseed, const int32_t* seed_atoms, const double* seed_coef, int lld, double a, double b,
                                      double* mu_n) {
    int rc = check_ready(h, "rsrec_chebyshev");
    if (rc) return rc;
    if (nchains < 0 || nseed < 1 || nseed > 8 || lld < 1 || !mu_n || (nchains > 0 && !seed_atoms) || a == 0.0) return fail(h, RSREC_ERR_ARG, "rsrec_chebyshev: bad argument");
    XFER(check_seeds(h, "rsrec_chebyshev", seed_atoms, (size_t)nchains * nseed, 1));
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    if (nchains == 0) return RSREC_OK;
    if (matrix_core_set(h)) return run_chebyshev<true>(h, nchains, nseed, seed_atoms, seed_coef, lld, a, b, mu_n);
    return run_chebyshev<false>(h, nchains, nseed, seed_atoms, seed_coef, lld, a, b, mu_n);
}

extern "C" int rsrec_chebyshev(rsrec_t* h, int nsites, const int32_t* seed_atoms, int lld, double a, double b, double* mu_n) {
    return rsrec_chebyshev_seeded(h, nsites, 1, seed_atoms, nullptr, lld, a, b, mu_n);
}

// ------------------------------------------------------------------------------------------------------------------
// Pair moments from one chain per atom (kernels_fan.hpp): a sibling of run_chebyshev on the same RecursionCall / recursion_batch set-up
namespace {

// Sources, gathered blocks and pair records of a call.  Sources ascend by atom; a source's entries follow each other, its own block first.
struct FanPlan {
    std::vector<int32_t> sources;          // 1-based atoms, as recursion_batch takes seeds
    std::vector<FanEntry> entries;
    std::vector<int> ent_begin;            // first entry of every source, and the total behind the last
    std::vector<FanPair> pairs;
};
void fan_plan(const rsrec_t* h, int npairs, const int32_t* ijpair, int both_ends, int nlev, FanPlan& F) {
    for (int p = 0; p < npairs; ++p) {
        F.sources.push_back(ijpair[2 * p]);
        if (both_ends) F.sources.push_back(ijpair[2 * p + 1]);
    }
    std::sort(F.sources.begin(), F.sources.end());
    F.sources.erase(std::unique(F.sources.begin(), F.sources.end()), F.sources.end());
    const int nsrc = (int)F.sources.size();
    auto source_of = [&](int atom1) { return (int)(std::lower_bound(F.sources.begin(), F.sources.end(), atom1) - F.sources.begin()); };
    std::vector<std::vector<int>> targets(nsrc);                 // 0-based atoms, the source itself first
    for (int s = 0; s < nsrc; ++s) targets[s].push_back(F.sources[s] - 1);
    auto slot_of = [&](int s, int atom0) {                       // position of a target in its source's list, appended when new
        auto& T = targets[s];
        const auto it = std::find(T.begin(), T.end(), atom0);
        if (it != T.end()) return (int)(it - T.begin());
        T.push_back(atom0);
        return (int)T.size() - 1;
    };
    std::vector<std::array<int, 4>> local(npairs);               // (source, slot) of ji and ij
    for (int p = 0; p < npairs; ++p) {
        const int i = ijpair[2 * p], j = ijpair[2 * p + 1];
        const int si = source_of(i);
        local[p] = {si, slot_of(si, j - 1), -1, -1};
        if (both_ends && i != j) { const int sj = source_of(j); local[p][2] = sj; local[p][3] = slot_of(sj, i - 1); }
    }
    F.ent_begin.assign(nsrc + 1, 0);
    std::vector<int> dist;
    for (int s = 0; s < nsrc; ++s) {
        F.ent_begin[s] = (int)F.entries.size();
        const int seed = F.sources[s] - 1;
        region_levels(lattice_view(h), &seed, 1, nlev, dist);
        for (int atom0 : targets[s]) F.entries.push_back(FanEntry{s, atom0, dist[atom0], atom0 == F.sources[s] - 1 ? 1 : 0});
    }
    F.ent_begin[nsrc] = (int)F.entries.size();
    F.pairs.resize(npairs);
    for (int p = 0; p < npairs; ++p) {
        const int i = ijpair[2 * p], j = ijpair[2 * p + 1];
        FanPair& P = F.pairs[p];
        P.ii = F.ent_begin[local[p][0]];
        P.ji = F.ent_begin[local[p][0]] + local[p][1];
        P.ij = P.jj = -1;
        if (i == j) P.mode = 0;
        else if (!both_ends) P.mode = 1;
        else { P.mode = 2; P.ij = F.ent_begin[local[p][2]] + local[p][3]; P.jj = F.ent_begin[local[p][2]]; }
    }
}

// VALU set: LayoutCM vectors; the matrix-core set always takes k_spmm5 on CI vectors here (the new vector is formed in its epilogue)
template <bool MFMA>
int run_pairs_direct(rsrec_t* h, int npairs, const int32_t* ijpair, int lld, double a, double b, int both_ends, double* mu_n, double* m_pair) {
    const bool hoh = h->hoh != 0;
    const int napply = 2 * lld + 1;                              // psi_1 .. psi_{2 lld + 1}: moment n + 1 is a block of psi_n
    const int nmom = 2 * lld + 2;
    FanPlan F;
    RecursionCall RC = recursion_call(h, MFMA, 0, 1, napply);
    fan_plan(h, npairs, ijpair, both_ends, RC.nlev, F);
    const int nsrc = RC.nchains = (int)F.sources.size(), nent = (int)F.entries.size();
    if (MFMA) RC.ci = 1;
    const size_t velems = RC.velems, mstride = (size_t)nmom * BLK;
    // resident outputs first, the batch is planned from what is left (see run_chebyshev)
    drop_resident(h);
    HIPCK(h, h->d_mu.reserve((size_t)4 * npairs * mstride * sizeof(double2)));
    HIPCK(h, h->d_fan.reserve((size_t)nent * mstride * sizeof(double2)));
    const size_t ent_bytes = (size_t)nent * sizeof(FanEntry), pair_off = (ent_bytes + 255) / 256 * 256;
    HIPCK(h, h->d_fan_tab.reserve(pair_off + (size_t)npairs * sizeof(FanPair)));
    if (m_pair) HIPCK(h, h->d_mpair.reserve((size_t)2 * npairs * mstride * sizeof(double2)));
    XFER(recursion_begin(h, RC, MFMA ? (hoh ? 5 : 4) : (hoh ? 4 : 3), MFMA ? 3 : -1, 1));
    XFER(xfer_h2d(h, h->d_fan_tab.p, F.entries.data(), ent_bytes));
    XFER(xfer_h2d(h, static_cast<char*>(h->d_fan_tab.p) + pair_off, F.pairs.data(), (size_t)npairs * sizeof(FanPair)));
    const FanEntry* d_ent = h->d_fan_tab.as<FanEntry>();
    const FanPair* d_pairs = reinterpret_cast<const FanPair*>(static_cast<const char*>(h->d_fan_tab.p) + pair_off);
    double2* img = h->d_fan.as<double2>();
    for (int c0 = 0; c0 < nsrc; c0 += RC.B) {
        const int nb = std::min(RC.B, nsrc - c0);
        const int e0 = F.ent_begin[c0], ne = F.ent_begin[c0 + nb] - e0;
        RecursionBatch bt;
        XFER(recursion_batch(h, RC, F.sources.data(), nullptr, c0, nb, bt));
        XFER(chain_level_loop(h, RC, bt, a, b, [&](const double* vec, int level, int n) {
            if (MFMA) k_fan_gather<LayoutCI><<<ne, FAN_THREADS, 0, h->stream>>>(vec, velems, d_ent, e0, c0, level, n, nmom, img, h->d_status.as<int>());
            else k_fan_gather<LayoutCM><<<ne, FAN_THREADS, 0, h->stream>>>(vec, velems, d_ent, e0, c0, level, n, nmom, img, h->d_status.as<int>());
        }));
    }
    double2* mu = h->d_mu.as<double2>();
    double2* mp = m_pair ? h->d_mpair.as<double2>() : nullptr;
    for (int q0 = 0; q0 < npairs; q0 += 32768) {                 // (grid.y holds 65535 at most)
        const int nq = std::min(32768, npairs - q0);
        k_fan_pack<<<dim3(nmom, nq), FAN_THREADS, 0, h->stream>>>(img, d_pairs + q0, nmom, mu + (size_t)4 * q0 * mstride, mp ? mp + (size_t)2 * q0 * mstride : nullptr);
    }
    HIPCK(h, hipGetLastError());
    XFER(xfer_d2h(h, mu_n, mu, (size_t)4 * npairs * mstride * sizeof(double2)));
    if (m_pair) XFER(xfer_d2h(h, m_pair, mp, (size_t)2 * npairs * mstride * sizeof(double2)));
    XFER(recursion_end(h, RC, 2, lld, true));
    h->res_n = 4 * npairs;                                       // what a seeded call of 4 npairs chains leaves
    return RSREC_OK;
}

}  // namespace

extern "C" int rsrec_chebyshev_pairs_direct(rsrec_t* h, int npairs, const int32_t* ijpair, int lld, double a, double b, int both_ends, double* mu_n,
                                            double* m_pair) {
    int rc = check_ready(h, "rsrec_chebyshev_pairs_direct");
    if (rc) return rc;
    if (npairs < 0 || lld < 1 || a == 0.0 || (npairs > 0 && (!ijpair || !mu_n))) return fail(h, RSREC_ERR_ARG, "rsrec_chebyshev_pairs_direct: bad argument");
    XFER(check_seeds(h, "rsrec_chebyshev_pairs_direct", ijpair, (size_t)2 * npairs, 1));
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    if (npairs == 0) return RSREC_OK;
    if (matrix_core_set(h)) return run_pairs_direct<true>(h, npairs, ijpair, lld, a, b, both_ends ? 1 : 0, mu_n, m_pair);
    return run_pairs_direct<false>(h, npairs, ijpair, lld, a, b, both_ends ? 1 : 0, mu_n, m_pair);
}

// ------------------------------------------------------------------------------------------------------------------
// k-resolved moments from one chain per atom (kernels_bloch.hpp): a sibling of run_pairs_direct -- the same chain, and behind the seed and every
// H|psi> launch the Bloch sum of the vector just written instead of the gather of a few blocks
namespace {

struct BlochCall {
    int nsrc, lld, nk, ngroup;
    const int32_t *sources, *group;
    double a, b;
    const double *cr, *kpt;
    BlochGeom G;
    double* s_k;
};

// The lists of a batch's chains as BlochLists takes them: per chain one segment per group, the group's atoms sorted by (level at which the
// atom joins the chain's region, atom); atoms the region never reaches are left out.  maxcnt[group][level]: the longest list of the batch.
// join[chain][kk]: that level for every atom on a list, INT_MAX for the others (the accumulation pass of run_bloch_map walks the atoms in order).
struct BlochBatchLists { std::vector<int> list, seg_off, count, tot, maxcnt, join; };
void bloch_lists(const rsrec_t* h, const BlochCall& A, int c0, int nb, int nlev, BlochBatchLists& T) {
    const int kk = h->kk, ng = A.ngroup;
    T.list.assign((size_t)nb * kk, 0); T.seg_off.assign((size_t)nb * ng, 0); T.count.assign((size_t)nb * ng * nlev, 0);
    T.tot.assign(nb, 0); T.maxcnt.assign((size_t)ng * nlev, 0); T.join.assign((size_t)nb * kk, INT_MAX);
    std::vector<int> dist, fill((size_t)ng * nlev);
    for (int c = 0; c < nb; ++c) {
        const int seed = A.sources[c0 + c] - 1;
        region_levels(lattice_view(h), &seed, 1, nlev, dist);
        int* cnt = T.count.data() + (size_t)c * ng * nlev;
        for (int j = 0; j < kk; ++j) {
            const int g = A.group ? A.group[j] : 1;
            if (g > 0 && dist[j] >= 0) cnt[(size_t)(g - 1) * nlev + dist[j]] += 1;
        }
        int off = 0;                                             // (group, level) buckets in order: atoms ascend inside a bucket
        for (int g = 0; g < ng; ++g) {
            T.seg_off[(size_t)c * ng + g] = off;
            for (int l = 0; l < nlev; ++l) { fill[(size_t)g * nlev + l] = off; off += cnt[(size_t)g * nlev + l]; }
        }
        T.tot[c] = off;
        for (int j = 0; j < kk; ++j) {
            const int g = A.group ? A.group[j] : 1;
            if (g > 0 && dist[j] >= 0) { T.list[(size_t)c * kk + fill[(size_t)(g - 1) * nlev + dist[j]]++] = j; T.join[(size_t)c * kk + j] = dist[j]; }
        }
        for (int g = 0; g < ng; ++g) {
            int run = 0;
            for (int l = 0; l < nlev; ++l) {
                run += cnt[(size_t)g * nlev + l];
                cnt[(size_t)g * nlev + l] = run;
                T.maxcnt[(size_t)g * nlev + l] = std::max(T.maxcnt[(size_t)g * nlev + l], run);
            }
        }
    }
}

// VALU set: LayoutCM vectors; the matrix-core set takes k_spmm5 on CI vectors, as run_pairs_direct does
template <bool MFMA>
int run_bloch(rsrec_t* h, const BlochCall& A) {
    const bool hoh = h->hoh != 0;
    const int kk = h->kk, nsrc = A.nsrc, nk = A.nk, ng = A.ngroup;
    const int napply = 2 * A.lld + 1, nmom = 2 * A.lld + 2;
    const int mpad = (2 * nk + BLOCH_MROWS - 1) / BLOCH_MROWS * BLOCH_MROWS, mchunk = std::min(mpad, BLOCH_MCHUNK);
    const size_t nimg = (size_t)nk * ng * nsrc, mstride = (size_t)nmom * BLK;
    RecursionCall RC = recursion_call(h, MFMA, nsrc, 1, napply);
    if (MFMA) RC.ci = 1;
    const size_t velems = RC.velems;
    // the resident image first, the batch is planned from what is left (see run_chebyshev)
    drop_resident(h);
    HIPCK(h, h->d_mu.reserve(nimg * mstride * sizeof(double2)));
    HIPCK(h, h->d_bloch_geo.reserve((size_t)3 * (kk + nk) * sizeof(double)));
    // per chain, sized with the work vectors (the buffer recursion_begin reserves for per-chain extras): the phase table and the partials
    const size_t tab_doubles = (size_t)kk * mpad, part_doubles = (size_t)BLOCH_MAXSPLIT * mchunk * BLD;
    XFER(recursion_begin(h, RC, MFMA ? (hoh ? 5 : 4) : (hoh ? 4 : 3), MFMA ? 3 : -1, 1, tab_doubles + part_doubles));
    double* table = h->d_gram.as<double>();
    double* partial = table + (size_t)RC.B * tab_doubles;
    double *d_cr = h->d_bloch_geo.as<double>(), *d_kpt = d_cr + (size_t)3 * kk;
    XFER(xfer_h2d(h, d_cr, A.cr, (size_t)3 * kk * sizeof(double)));
    XFER(xfer_h2d(h, d_kpt, A.kpt, (size_t)3 * nk * sizeof(double)));
    const size_t n_list = (size_t)RC.B * kk, n_off = (size_t)RC.B * ng, n_cnt = n_off * RC.nlev;
    HIPCK(h, h->d_bloch_tab.reserve((n_list + n_off + n_cnt + RC.B) * sizeof(int)));
    int *d_list = h->d_bloch_tab.as<int>(), *d_off = d_list + n_list, *d_cnt = d_off + n_off, *d_tot = d_cnt + n_cnt;
    double2* mu = h->d_mu.as<double2>();
    std::vector<std::pair<hipEvent_t, hipEvent_t>> bloch_ev;
    BlochBatchLists T;
    for (int c0 = 0; c0 < nsrc; c0 += RC.B) {
        const int nb = std::min(RC.B, nsrc - c0);
        RecursionBatch bt;
        XFER(recursion_batch(h, RC, A.sources, nullptr, c0, nb, bt));
        bloch_lists(h, A, c0, nb, RC.nlev, T);
        XFER(xfer_h2d(h, d_list, T.list.data(), (size_t)nb * kk * sizeof(int)));
        XFER(xfer_h2d(h, d_off, T.seg_off.data(), (size_t)nb * ng * sizeof(int)));
        XFER(xfer_h2d(h, d_cnt, T.count.data(), (size_t)nb * ng * RC.nlev * sizeof(int)));
        XFER(xfer_h2d(h, d_tot, T.tot.data(), (size_t)nb * sizeof(int)));
        const BlochLists BL{d_list, d_off, d_cnt, kk, ng, RC.nlev};
        const int* d_src = h->d_seed.as<int>();                  // (one seed per chain: the batch's 0-based source atoms)
        {
            hipEvent_t e0 = next_event(h);
            const int maxtot = *std::max_element(T.tot.begin(), T.tot.end());
            const unsigned gx = (unsigned)std::min<size_t>(4096, ((size_t)maxtot * (mpad / 2) + 255) / 256);
            k_bloch_phase<<<dim3(std::max(1u, gx), nb), 256, 0, h->stream>>>(BL, d_tot, d_src, d_cr, d_kpt, nk, mpad, A.G, table);
            bloch_ev.emplace_back(e0, next_event(h));
        }
        // the Bloch sums of the vector of order n (region level `level`) into moment n of the batch's images
        auto bloch_pass = [&](const double* vec, int level, int n) {
            hipEvent_t e0 = next_event(h);
            if (MFMA) k_bloch_diverge<LayoutCI><<<nb, BLOCH_THREADS, 0, h->stream>>>(vec, velems, d_src, h->d_status.as<int>());
            else k_bloch_diverge<LayoutCM><<<nb, BLOCH_THREADS, 0, h->stream>>>(vec, velems, d_src, h->d_status.as<int>());
            for (int g = 0; g < ng; ++g) {
                if (!MFMA) { k_bloch_valu<LayoutCM><<<dim3(nk, nb), BLOCH_THREADS, 0, h->stream>>>(BL, g, level, vec, velems, table, mpad, nk, c0, n, nmom, mu); continue; }
                const int splits = bloch_splits(T.maxcnt[(size_t)g * RC.nlev + level]);
                for (int m0 = 0; m0 < mpad; m0 += BLOCH_MCHUNK) {
                    const int mrows = std::min(BLOCH_MCHUNK, mpad - m0), q0 = m0 / 2, nq = std::min(nk - q0, mrows / 2);
                    k_bloch_mfma<<<dim3(BLOCH_NPB * (mrows / BLOCH_MROWS), splits, nb), BLOCH_WAVES * 64, 0, h->stream>>>(BL, g, level, vec, velems, table, mpad, m0, mrows, partial);
                    k_bloch_reduce<<<dim3(nq, nb), BLOCH_THREADS, 0, h->stream>>>(BL, g, level, partial, mrows, q0, nk, c0, n, nmom, mu);
                }
            }
            bloch_ev.emplace_back(e0, next_event(h));
        };
        XFER(chain_level_loop(h, RC, bt, A.a, A.b, bloch_pass));   // (it ends idle: the next batch's uploads reuse the lists too)
    }
    if (A.s_k) XFER(xfer_d2h(h, A.s_k, mu, nimg * mstride * sizeof(double2)));
    const int rc = recursion_end(h, RC, 2, A.lld, false);
    h->t_rest_ms = 0;                                            // out[5]: the phase table and the Bloch passes alone
    for (auto& pr : bloch_ev) h->t_rest_ms += ev_ms(pr.first, pr.second);
    h->d_gram.release();                                         // (tables and partials: not left behind as another call's Gram buffer)
    if (rc) return rc;
    h->res_n = (int)nimg;                                        // what an rsrec_chebyshev call of nsrc * ngroup * nk sites leaves
    return RSREC_OK;
}

}  // namespace

namespace {

// The argument checks rsrec_chebyshev_bloch and rsrec_chebyshev_bloch_map share (nk_max: the call's own limit); fills the cell's geometry
int bloch_check_args(rsrec_t* h, const char* who, int nsrc, const int32_t* sources, int lld, double a, const double* cr, const double* cell, int nk, int nk_max,
                     const double* kpt, int ngroup, const int32_t* group, BlochGeom& G) {
    if (nsrc < 0 || lld < 1 || a == 0.0) return fail(h, RSREC_ERR_ARG, "%s: nsrc < 0, lld < 1 or a == 0", who);
    if (nk < 1 || nk > nk_max) return fail(h, RSREC_ERR_ARG, "%s: nk = %d outside 1..%d", who, nk, nk_max);
    if (ngroup < 1 || ngroup > RSREC_BLOCH_NGROUP_MAX) return fail(h, RSREC_ERR_ARG, "%s: ngroup = %d outside 1..%d", who, ngroup, RSREC_BLOCH_NGROUP_MAX);
    if (!cr || !kpt || (nsrc > 0 && !sources)) return fail(h, RSREC_ERR_ARG, "%s: NULL sources, cr or kpt", who);
    if (!group && ngroup != 1) return fail(h, RSREC_ERR_ARG, "%s: ngroup = %d needs a group array", who, ngroup);
    if (group)
        for (int j = 0; j < h->kk; ++j)
            if (group[j] < 0 || group[j] > ngroup) return fail(h, RSREC_ERR_ARG, "%s: group(%d) = %d outside 0..%d", who, j + 1, group[j], ngroup);
    XFER(check_seeds(h, who, sources, (size_t)nsrc, 1));
    if ((size_t)nk * ngroup * (size_t)nsrc > (size_t)INT32_MAX) return fail(h, RSREC_ERR_ARG, "%s: nk * ngroup * nsrc exceeds the index range", who);
    G = BlochGeom{};
    G.wrap = cell ? 1 : 0;
    if (cell) {
        const double* c = cell;                                  // column-major: c[3 col + row]
        const double cof[9] = {c[4] * c[8] - c[5] * c[7], c[5] * c[6] - c[3] * c[8], c[3] * c[7] - c[4] * c[6],
                               c[7] * c[2] - c[8] * c[1], c[8] * c[0] - c[6] * c[2], c[6] * c[1] - c[7] * c[0],
                               c[1] * c[5] - c[2] * c[4], c[2] * c[3] - c[0] * c[5], c[0] * c[4] - c[1] * c[3]};
        const double det = c[0] * cof[0] + c[1] * cof[1] + c[2] * cof[2];
        double len = 1.0;
        for (int v = 0; v < 3; ++v) len *= std::sqrt(c[3 * v] * c[3 * v] + c[3 * v + 1] * c[3 * v + 1] + c[3 * v + 2] * c[3 * v + 2]);
        if (!std::isfinite(det) || !(std::fabs(det) > 1e-12 * len)) return fail(h, RSREC_ERR_ARG, "%s: singular cell", who);
        // inv(row i, col j) = cof(j, i) / det with cof[3 j + i] the cofactor of c(i, j) as laid out above
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) { G.cell[3 * j + i] = c[3 * j + i]; G.inv[3 * j + i] = cof[3 * i + j] / det; }
    }
    return RSREC_OK;
}

}  // namespace

extern "C" int rsrec_chebyshev_bloch(rsrec_t* h, int nsrc, const int32_t* sources, int lld, double a, double b, const double* cr, const double* cell,
                                     int nk, const double* kpt, int ngroup, const int32_t* group, double* s_k) {
    const char* who = "rsrec_chebyshev_bloch";
    int rc = check_ready(h, who);
    if (rc) return rc;
    BlochCall A{nsrc, lld, nk, ngroup, sources, group, a, b, cr, kpt, BlochGeom{}, s_k};
    XFER(bloch_check_args(h, who, nsrc, sources, lld, a, cr, cell, nk, RSREC_BLOCH_NK_MAX, kpt, ngroup, group, A.G));
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    if (nsrc == 0) return RSREC_OK;
    return matrix_core_set(h) ? run_bloch<true>(h, A) : run_bloch<false>(h, A);
}

// ------------------------------------------------------------------------------------------------------------------
// Functions of H at many k-points from one chain per atom (kernels_blochmap.hpp): a sibling of run_bloch on the same chain and the same lists --
// behind the seed and every H|psi> launch the vector is added into ne weighted sums Y_e instead of being Bloch-summed, and ONE Bloch sum per
// energy follows the last order, a chunk of k-points at a time
namespace {

struct BlochMapCall {
    BlochCall B;                 // sources, window, geometry, k-points and groups as rsrec_chebyshev_bloch takes them (s_k unused)
    int ne;
    const double* w;             // complex (2 lld + 2, ne)
    double *g_k, *a_k;
};

template <bool MFMA>
int run_bloch_map(rsrec_t* h, const BlochMapCall& M) {
    const BlochCall& A = M.B;
    const bool hoh = h->hoh != 0, two = h->opt_blochmap_orders != 1;
    const int kk = h->kk, nsrc = A.nsrc, nk = A.nk, ng = A.ngroup, ne = M.ne;
    const int napply = 2 * A.lld + 1, nmom = 2 * A.lld + 2;
    // k-points per chunk of the final sums: one launch's rows of the phase matrix unless the option says otherwise.  A point's bits do not
    // depend on it: the rows of the phase matrix are independent in the product.
    const int kchunk = (int)std::min<long>(nk, h->opt_blochmap_kchunk > 0 ? h->opt_blochmap_kchunk : BLOCH_MCHUNK / 2);
    auto pad_rows = [](int nq) { return (2 * nq + BLOCH_MROWS - 1) / BLOCH_MROWS * BLOCH_MROWS; };
    const int mpad_max = pad_rows(kchunk);
    RecursionCall RC = recursion_call(h, MFMA, nsrc, 1, napply);
    if (MFMA) RC.ci = 1;
    const size_t velems = RC.velems;
    // an output in device memory is written in place by the kernels; a host array gets the chunk's images from a staging buffer
    const bool g_dev = M.g_k && is_device_ptr(M.g_k), a_dev = M.a_k && is_device_ptr(M.a_k);
    drop_resident(h);                                            // the call leaves no image, and what an earlier call left goes with the buffers
    HIPCK(h, h->d_bloch_geo.reserve((size_t)3 * (kk + nk) * sizeof(double)));
    HIPCK(h, h->d_map_w.reserve((size_t)nmom * ne * sizeof(double2)));
    // per chain, charged in the batch plan with the work vectors: the accumulators, the phase table and the partials of ONE chunk, its staged images
    const size_t acc_doubles = (size_t)ne * velems, tab_doubles = (size_t)kk * mpad_max, part_doubles = (size_t)BLOCH_MAXSPLIT * std::min(mpad_max, BLOCH_MCHUNK) * BLD;
    const size_t sg_doubles = g_dev ? 0 : (size_t)kchunk * ng * ne * 2 * BLK, sa_doubles = M.a_k && !a_dev ? (size_t)kchunk * ng * ne * NB : 0;
    XFER(recursion_begin(h, RC, MFMA ? (hoh ? 5 : 4) : (hoh ? 4 : 3), MFMA ? 3 : -1, 1, acc_doubles + tab_doubles + part_doubles + sg_doubles + sa_doubles));
    double* Y = h->d_gram.as<double>();
    double* table = Y + (size_t)RC.B * acc_doubles;
    double* partial = table + (size_t)RC.B * tab_doubles;
    double* stage_g = partial + (size_t)RC.B * part_doubles;
    double* stage_a = stage_g + (size_t)RC.B * sg_doubles;
    double2* g_out = g_dev ? reinterpret_cast<double2*>(M.g_k) : reinterpret_cast<double2*>(stage_g);
    double* a_out = a_dev ? M.a_k : stage_a;
    double *d_cr = h->d_bloch_geo.as<double>(), *d_kpt = d_cr + (size_t)3 * kk;
    XFER(xfer_h2d(h, d_cr, A.cr, (size_t)3 * kk * sizeof(double)));
    XFER(xfer_h2d(h, d_kpt, A.kpt, (size_t)3 * nk * sizeof(double)));
    XFER(xfer_h2d(h, h->d_map_w.p, M.w, (size_t)nmom * ne * sizeof(double2)));
    const double2* d_w = h->d_map_w.as<double2>();
    const size_t n_list = (size_t)RC.B * kk, n_off = (size_t)RC.B * ng, n_cnt = n_off * RC.nlev;
    HIPCK(h, h->d_bloch_tab.reserve((2 * n_list + n_off + n_cnt + RC.B) * sizeof(int)));
    int *d_list = h->d_bloch_tab.as<int>(), *d_off = d_list + n_list, *d_cnt = d_off + n_off, *d_tot = d_cnt + n_cnt, *d_join = d_tot + RC.B;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> map_ev[3];    // accumulation passes | phase tables | final sums
    BlochBatchLists T;
    const int last = RC.nlev - 1;                                // the region level of the last order
    const dim3 acc_grid((unsigned)(((size_t)kk * BLK + MAP_WG_ELEMS - 1) / MAP_WG_ELEMS), 1);
    for (int c0 = 0; c0 < nsrc; c0 += RC.B) {
        const int nb = std::min(RC.B, nsrc - c0);
        RecursionBatch bt;
        XFER(recursion_batch(h, RC, A.sources, nullptr, c0, nb, bt));
        bloch_lists(h, A, c0, nb, RC.nlev, T);
        XFER(xfer_h2d(h, d_list, T.list.data(), (size_t)nb * kk * sizeof(int)));
        XFER(xfer_h2d(h, d_off, T.seg_off.data(), (size_t)nb * ng * sizeof(int)));
        XFER(xfer_h2d(h, d_cnt, T.count.data(), (size_t)nb * ng * RC.nlev * sizeof(int)));
        XFER(xfer_h2d(h, d_tot, T.tot.data(), (size_t)nb * sizeof(int)));
        XFER(xfer_h2d(h, d_join, T.join.data(), (size_t)nb * kk * sizeof(int)));
        const BlochLists BL{d_list, d_off, d_cnt, kk, ng, RC.nlev};
        const int* d_src = h->d_seed.as<int>();                  // (one seed per chain: the batch's 0-based source atoms)
        HIPCK(h, hipMemsetAsync(Y, 0, (size_t)nb * acc_doubles * sizeof(double), h->stream));
        // Y_e += w(n, e) psi_n on the atoms inside at the order's level; with two orders per pass the odd orders add the vector before them too
        const double* prev = nullptr;
        int prev_level = 0;
        auto accum_pass = [&](const double* vec, int level, int n) {
            hipEvent_t e0 = next_event(h);
            if (MFMA) k_bloch_diverge<LayoutCI><<<nb, BLOCH_THREADS, 0, h->stream>>>(vec, velems, d_src, h->d_status.as<int>());
            else k_bloch_diverge<LayoutCM><<<nb, BLOCH_THREADS, 0, h->stream>>>(vec, velems, d_src, h->d_status.as<int>());
            const dim3 grid(acc_grid.x, nb);
            const double2 *x = reinterpret_cast<const double2*>(vec), *xo = reinterpret_cast<const double2*>(prev);
            if (!two) k_map_accum<false><<<grid, MAP_THREADS, 0, h->stream>>>(d_join, kk, level, level, x, x, velems / 2, d_w, n, nmom, ne, reinterpret_cast<double2*>(Y));
            else if (n & 1) k_map_accum<true><<<grid, MAP_THREADS, 0, h->stream>>>(d_join, kk, level, prev_level, x, xo, velems / 2, d_w, n, nmom, ne, reinterpret_cast<double2*>(Y));
            prev = vec; prev_level = level;
            map_ev[0].emplace_back(e0, next_event(h));
        };
        XFER(chain_level_loop(h, RC, bt, A.a, A.b, accum_pass));  // (the last order, 2 lld + 1, is odd: every order has been added when it ends)
        for (int q0 = 0; q0 < nk; q0 += kchunk) {
            const int nq = std::min(kchunk, nk - q0), mpad = pad_rows(nq);
            hipEvent_t e0 = next_event(h);
            const int maxtot = *std::max_element(T.tot.begin(), T.tot.end());
            const unsigned gx = (unsigned)std::min<size_t>(4096, ((size_t)maxtot * (mpad / 2) + 255) / 256);
            k_bloch_phase<<<dim3(std::max(1u, gx), nb), 256, 0, h->stream>>>(BL, d_tot, d_src, d_cr, d_kpt + (size_t)3 * q0, nq, mpad, A.G, table);
            hipEvent_t e1 = next_event(h);
            map_ev[1].emplace_back(e0, e1);
            const MapSlot gs = g_dev ? MapSlot{q0, nk, c0} : MapSlot{0, nq, 0}, as = a_dev ? MapSlot{q0, nk, c0} : MapSlot{0, nq, 0};
            for (int e = 0; e < ne; ++e) {
                const double* vec = Y + (size_t)e * velems;      // energy e of chain c: Y + (c ne + e) velems
                for (int g = 0; g < ng; ++g) {
                    if (!MFMA) {
                        k_bloch_valu<LayoutCM><<<dim3(nq, nb), BLOCH_THREADS, 0, h->stream>>>(BL, g, last, vec, acc_doubles, table, mpad, gs.nk, gs.c0, e, ne, g_out + (size_t)gs.q0 * ne * BLK);
                        continue;
                    }
                    const int splits = bloch_splits(T.maxcnt[(size_t)g * RC.nlev + last]);
                    for (int m0 = 0; m0 < mpad; m0 += BLOCH_MCHUNK) {
                        const int mrows = std::min(BLOCH_MCHUNK, mpad - m0), nqq = std::min(nq - m0 / 2, mrows / 2);
                        k_bloch_mfma<<<dim3(BLOCH_NPB * (mrows / BLOCH_MROWS), splits, nb), BLOCH_WAVES * 64, 0, h->stream>>>(BL, g, last, vec, acc_doubles, table, mpad, m0, mrows, partial);
                        k_bloch_reduce<<<dim3(nqq, nb), BLOCH_THREADS, 0, h->stream>>>(BL, g, last, partial, mrows, gs.q0 + m0 / 2, gs.nk, gs.c0, e, ne, g_out);
                    }
                }
            }
            if (M.a_k) k_map_diag<<<dim3(nq, ng, nb), MAP_DIAG_THREADS, 0, h->stream>>>(g_out, gs, a_out, as, ng, ne);
            HIPCK(h, hipGetLastError());
            map_ev[2].emplace_back(e1, next_event(h));
            // the chunk's slice of a host array: per (chain, group) the chunk's points are contiguous on both sides
            for (int c = 0; c < nb; ++c)
                for (int g = 0; g < ng; ++g) {
                    const size_t from = (size_t)nq * (g + (size_t)ng * c) * ne, to = ((size_t)q0 + (size_t)nk * (g + (size_t)ng * (c0 + c))) * ne;
                    if (M.g_k && !g_dev) XFER(xfer_d2h(h, M.g_k + to * 2 * BLK, stage_g + from * 2 * BLK, (size_t)nq * ne * BLK * sizeof(double2)));
                    if (M.a_k && !a_dev) XFER(xfer_d2h(h, M.a_k + to * NB, stage_a + from * NB, (size_t)nq * ne * NB * sizeof(double)));
                }
        }
    }
    const int rc = recursion_end(h, RC, 0, A.lld, false);        // (res_kind 0: nothing stays resident)
    h->t_rest_ms = 0;                                            // out[5]: the three parts together
    for (int k = 0; k < 3; ++k) {
        for (auto& pr : map_ev[k]) h->t_map_ms[k] += ev_ms(pr.first, pr.second);
        h->t_rest_ms += h->t_map_ms[k];
    }
    h->d_gram.release();                                         // (accumulators, tables and partials: not left behind as another call's Gram buffer)
    return rc;
}

}  // namespace

extern "C" int rsrec_chebyshev_bloch_map(rsrec_t* h, int nsrc, const int32_t* sources, int lld, double a, double b, const double* cr, const double* cell,
                                         int nk, const double* kpt, int ngroup, const int32_t* group, int ne, const double* w, double* g_k, double* a_k) {
    const char* who = "rsrec_chebyshev_bloch_map";
    int rc = check_ready(h, who);
    if (rc) return rc;
    BlochMapCall M{BlochCall{nsrc, lld, nk, ngroup, sources, group, a, b, cr, kpt, BlochGeom{}, nullptr}, ne, w, g_k, a_k};
    XFER(bloch_check_args(h, who, nsrc, sources, lld, a, cr, cell, nk, RSREC_BLOCH_MAP_NK_MAX, kpt, ngroup, group, M.B.G));
    if (ne < 1 || ne > RSREC_BLOCH_MAP_NE_MAX) return fail(h, RSREC_ERR_ARG, "%s: ne = %d outside 1..%d", who, ne, RSREC_BLOCH_MAP_NE_MAX);
    if (!w) return fail(h, RSREC_ERR_ARG, "%s: NULL w", who);
    for (size_t q = 0; q < (size_t)2 * (2 * lld + 2) * ne; ++q)
        if (!std::isfinite(w[q])) return fail(h, RSREC_ERR_ARG, "%s: weight (%zu, %zu) is not finite", who, q / 2 % (2 * lld + 2) + 1, q / 2 / (2 * lld + 2) + 1);
    if (!g_k && !a_k) return fail(h, RSREC_ERR_ARG, "%s: g_k and a_k are both NULL", who);
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    if (nsrc == 0) return RSREC_OK;
    return matrix_core_set(h) ? run_bloch_map<true>(h, M) : run_bloch_map<false>(h, M);
}

// ------------------------------------------------------------------------------------------------------------------
// Products over the whole lattice: the stochastic Kubo double moments, the orbital moments, single products on caller arrays
namespace {

// An operator table of k_spmm5 from blocks on the host (2 BLK doubles each): `fill` gets blk(set, tau, slot), the pointer of class tau <
// nmax + ntype (per-atom classes first, then types) and slot <= nslots (the last: the extra on-site slot of two-input passes), and sets
// those that exist.  What the pointers refer to has to live until this returns.  A failure is reported as "`who`: ...".
template <class Fill>
int build_operator_table(rsrec_t* h, Spmm5Operator& op, int nset, const char* who, Fill&& fill) {
    const int ntau = h->nmax + h->ntype, nfs = h->nslots + 1;
    std::vector<const double*> blk((size_t)nset * ntau * nfs, nullptr);
    fill([&](int set, int tau, int slot) -> const double*& { return blk[((size_t)set * ntau + tau) * nfs + slot]; });
    const char* msg = op.build_custom(h->nslots, ntau, nset, blk);
    if (msg) return fail(h, RSREC_ERR_DEVICE, "%s: %s", who, msg);
    return RSREC_OK;
}

// Operator tables of a velocity-type operator (recursion.f90:587-784) into `op`: kubo_op[j] (output operator j; v_a is j = 0) or kubo_op_b (v_b).
//   set 0: V itself -- per-type blocks v_op(:,:,slot,type) for the bulk atoms; the reference has no velocity operator for the
//          per-atom (impurity) region yet (":591 NOT YET IMPLEMENTED"): those rows of V psi are zero, as there.
//   set 1 (hoh): -vo_op(:,:,slot,type) for slots >= 2 and the identity in the extra slot, so that one pass over h psi with V psi as
//          second input gives  V psi - sum_{slot >= 2} vo_slot (h psi)_nbr  (velo_hoh_vec_matmul :750-776; its on-site vo term is
//          commented out in the reference, its e_nu / l.s terms are zero).
int build_kubo_operator(rsrec_t* h, Spmm5Operator& op, const double* v, const double* vo) {
    const int nset = h->hoh ? 2 : 1;
    const size_t B = 2 * (size_t)BLK;
    std::vector<double> neg((size_t)h->ntype * h->nslots * B, 0.0), ident(B, 0.0);
    for (int d = 0; d < NB; ++d) ident[2 * (d + NB * d)] = 1.0;
    return build_operator_table(h, op, nset, "rsrec_kubo_moments", [&](auto&& blk) {
        for (int t = 0; t < h->ntype; ++t)
            for (int s = 0; s < h->nslots; ++s) {
                blk(0, h->nmax + t, s) = v + B * (s + (size_t)h->hslots * t);
                if (nset > 1 && s >= 1) {
                    double* d = neg.data() + B * (s + (size_t)h->nslots * t);
                    const double* src = vo + B * (s + (size_t)h->hslots * t);
                    for (size_t e = 0; e < B; ++e) d[e] = -src[e];
                    blk(1, h->nmax + t, s) = d;
                }
            }
        if (nset > 1)
            for (int t = 0; t < h->ntype; ++t) blk(1, h->nmax + t, h->nslots) = ident.data();
    });
}

// h restricted to the bulk atoms (psi1 of velo_hoh_vec_matmul :727-741 is only formed for k > nmax)
int build_kubo_hbulk(rsrec_t* h) {
    const size_t B = 2 * (size_t)BLK;
    return build_operator_table(h, h->kubo_hbulk, 1, "rsrec_kubo_moments", [&](auto&& blk) {
        for (int t = 0; t < h->ntype; ++t)
            for (int s = 0; s < h->nslots; ++s) blk(0, h->nmax + t, s) = h->host_ee.data() + B * (s + (size_t)h->hslots * t);
    });
}

// h as ham_vec_matmul applies it (recursion.f90:913-977): per-type blocks ee (per-atom hall for the impurity region) with l.s added to
// the on-site block -- whatever hamiltonian%hoh says.  Without hoh that is set 0 of s5_op; with hoh a table of its own.
int build_plain_operator(rsrec_t* h) {
    const int ntau = h->nmax + h->ntype;
    const size_t B = 2 * (size_t)BLK;
    std::vector<double> onsite((size_t)ntau * B);
    return build_operator_table(h, h->orb_plain, 1, "plain operator table", [&](auto&& blk) {
        for (int tau = 0; tau < ntau; ++tau) {
            const int ty = tau < h->nmax ? h->iz0[tau] : tau - h->nmax;
            const double* base = tau < h->nmax ? h->host_hall.data() + B * (size_t)h->hslots * tau : h->host_ee.data() + B * (size_t)h->hslots * (tau - h->nmax);
            for (size_t e = 0; e < B; ++e) onsite[(size_t)tau * B + e] = base[e] + h->host_lsham[B * ty + e];
            blk(0, tau, 0) = onsite.data() + (size_t)tau * B;
            for (int s = 1; s < h->nslots; ++s) blk(0, tau, s) = base + B * s;
        }
    });
}

// What rsrec_kubo_moments, rsrec_orbital_moments and rsrec_apply_operator share, as the recursion drivers share RecursionCall: every product
// is one k_spmm5 launch (two with hoh) over the list of ALL atoms -- one order row, level 0, shared by the chains of the launch -- on whole
// vectors side by side in buffer slots of `chains_per_slot` chains.  The call reads:  reserve -> whole_lattice_begin -> set the temporaries ->
// ev_begin -> per batch { whole_lattice_batch; products } -> whole_lattice_end.
struct WholeLatticeCall {
    rsrec_t* h = nullptr;
    bool timed = false;                  // events around every launch and the flop accounting (false: rsrec_apply_operator, the call's span only)
    SpmmDims SD; ChainView CV; dim3 grid; const int* iz = nullptr;   // what launch_s5 takes (CV also k_mfma_adot)
    double *hps = nullptr, *p1 = nullptr, *p2 = nullptr;   // the caller's temporaries of the two-pass products (hoh): h psi; h_bulk psi and V psi
    hipEvent_t ev_begin = nullptr;       // start of the timed span: the caller records it once its uploads are done
    std::vector<std::pair<hipEvent_t, hipEvent_t>> hop_ev, rest_ev;   // every SpMM launch; what else a call times by itself (Kubo: the contractions)
    std::vector<std::tuple<const Spmm5Operator*, int, double>> req;   // required flops of a product with (operator, set): computed once per call
    double chain_launches = 0;           // whole-lattice products of the call: launches x chains in them
};

// The list of all atoms as the one region (cached like every region) and the launch shape for a full batch of `chains_per_slot` chains.
// `grouped`: the list padded into operator-class groups of 8, as k_spmm5 walks it (false: the VALU set's k_apply, rsrec_chebyshev_lattice).
int whole_lattice_begin(rsrec_t* h, WholeLatticeCall& W, int chains_per_slot, bool timed, bool grouped = true) {
    const int kk = h->kk;
    const size_t velems = (size_t)(kk + 1) * BLD;
    std::vector<int> all(kk);
    std::iota(all.begin(), all.end(), 0);
    XFER(upload_regions(h, all.data(), 1, kk, 1, 1, false, grouped));
    W.h = h; W.timed = timed;
    chain_views(h, velems, chains_per_slot, W.CV);
    W.SD = SpmmDims{kk, h->nslots, h->nmax, 1, chains_per_slot, W.CV.ostride, 0, velems, W.CV.obase, chains_per_slot};
    W.grid = s5_grid(h, dim3(256, (unsigned)chains_per_slot), 0);
    W.iz = h->d_iz.as<int>();
    return RSREC_OK;
}

// The launches of a batch of nb <= chains_per_slot chains (the last batch of a call may be short; the slots keep their width).
// The kernels find a chain's order row as chain / cpo (k_spmm5, k_mfma_adot): with one row and nb <= cpo that is row 0 whether cpo stays the
// slot's width (rsrec_kubo_moments) or follows the batch (rsrec_orbital_moments) -- the same memory either way.  The HOST side of launch_s5
// reads it too: only launches with cpo == 1 add to the executed-flop counter (and may take the class-run and octet forms), so a short batch of
// ONE chain counts under the second form and not under the first.  Hence the parameter: each caller keeps what it did, and the counters of
// rsrec_get_timing with them.
void whole_lattice_batch(WholeLatticeCall& W, int nb, bool cpo_follows_batch) {
    W.SD.nchains = nb;
    if (cpo_follows_batch) W.CV.cpo = W.SD.cpo = nb;
    W.grid = s5_grid(W.h, dim3(256, (unsigned)nb), 0);
}

// flops one whole-lattice product with operator (op, set) requires by its block structure (see required_hop_flops)
double whole_lattice_required_flops(const rsrec_t* h, const Spmm5Operator& op, int set) {
    double f = 0.0;
    const int ns = h->nslots;
    for (int i = 0; i < h->kk; ++i) {
        const int tau = i < h->nmax ? i : h->nmax + h->iz0[i];
        for (int s2 = 0; s2 < ns; ++s2)
            if (h->nbr[(size_t)i * ns + s2] >= 0) f += op.required_flops(set, tau, s2);
        f += op.required_flops(set, tau, ns);               // the extra on-site slot of two-input passes (0 if the class has none)
    }
    return f;
}

// one launch: out = op(set) in  [+ the extra slot's block on in2], through the epilogue
void whole_lattice_spmm(WholeLatticeCall& W, const Spmm5Operator& op, int set, const double* in, double* out, const double* in2, S5Epilogue epi = S5Epilogue()) {
    rsrec_t* h = W.h;
    hipEvent_t e0 = W.timed ? next_event(h) : nullptr;
    if (in2) launch_s5<true>(h, W.grid, W.SD, W.CV.order, W.CV.cum, W.iz, op, set, in, out, in2, nullptr, 0, epi);
    else launch_s5<false>(h, W.grid, W.SD, W.CV.order, W.CV.cum, W.iz, op, set, in, out, nullptr, nullptr, 0, epi);
    if (!W.timed) return;
    W.hop_ev.emplace_back(e0, next_event(h));
    double f = -1.0;
    for (auto& e : W.req) if (std::get<0>(e) == &op && std::get<1>(e) == set) f = std::get<2>(e);
    if (f < 0.0) { f = whole_lattice_required_flops(h, op, set); W.req.emplace_back(&op, set, f); }
    h->n_req_flop += f * W.SD.nchains;
    W.chain_launches += W.SD.nchains;
}
// out = H in   (ham_vec_matmul :913 / ham_hoh_vec_matmul :785 before their scale-and-shift), or with an epilogue the whole Chebyshev
// step  out = (H in - b in)/a  [* 2 - old]  (their scale-and-shift :968-970 and the caller's recurrence :1132-1136) in the same kernel
void whole_lattice_apply_h(WholeLatticeCall& W, const double* in, double* out, S5Epilogue epi = S5Epilogue()) {
    if (!W.h->hoh) { whole_lattice_spmm(W, W.h->s5_op, 0, in, out, nullptr, epi); return; }
    whole_lattice_spmm(W, W.h->s5_op, 0, in, W.hps, nullptr);
    whole_lattice_spmm(W, W.h->s5_op, 1, W.hps, out, in, epi);
}
// out = V in   (velo_vec_matmul :587 / velo_hoh_vec_matmul :656)
// in two halves, for several V on one `in`: h_bulk in -> p1 (hoh only; it does not depend on V), then out = V in from it
void whole_lattice_apply_v_prepare(WholeLatticeCall& W, const double* in) {
    if (W.h->hoh) whole_lattice_spmm(W, W.h->nmax > 0 ? W.h->kubo_hbulk : W.h->s5_op, 0, in, W.p1, nullptr);
}
void whole_lattice_apply_v_prepared(WholeLatticeCall& W, const Spmm5Operator& vop, const double* in, double* out) {
    if (!W.h->hoh) { whole_lattice_spmm(W, vop, 0, in, out, nullptr); return; }
    whole_lattice_spmm(W, vop, 0, in, W.p2, nullptr);
    whole_lattice_spmm(W, vop, 1, W.p1, out, W.p2);
}
void whole_lattice_apply_v(WholeLatticeCall& W, const Spmm5Operator& vop, const double* in, double* out) {
    whole_lattice_apply_v_prepare(W, in);
    whole_lattice_apply_v_prepared(W, vop, in, out);
}

// The three-term recurrence on whole vectors, H~ = (H - b)/a: with T_0(H~) x in `cur`, step(n) for n = 0, 1, 2, ... leaves T_n(H~) x in `cur`
// (n = 0: nothing to do) and T_{n-1}(H~) x in `old`; from n = 2 on the three buffers rotate, and `spare` is T_{n-2}(H~) x during the launch.
struct ChebyshevStepper {
    double *old, *cur, *spare;
    void rotate(int n) {                 // the buffers of step n >= 1, before its launch
        if (n == 1) std::swap(old, cur);
        else { double* o = spare; spare = old; old = cur; cur = o; }
    }
    void step(WholeLatticeCall& W, int n, double a, double b) {
        if (n == 0) return;
        rotate(n);
        whole_lattice_apply_h(W, old, cur, cheb_epilogue(n == 1, old, spare, a, b));
    }
};

// End of a call: the closing event, the stream, the timing.  Untimed calls report total_ms only.  Timed ones report every SpMM launch as hop_ms
// and hop_launches; rest_ms is total - hop (finish_timing) unless `rest_is_own_spans`: then it is the sum of rest_ev -- rsrec_kubo_moments'
// contractions, so that hop_ms + rest_ms < total_ms there -- and the work counters are in the reference's terms: every product is over the
// whole lattice, one block multiply per (atom, present slot).
int whole_lattice_end(rsrec_t* h, WholeLatticeCall& W, bool rest_is_own_spans = false) {
    hipEvent_t ev_end = next_event(h);
    HIPCK(h, hipStreamSynchronize(h->stream));
    HIPCK(h, hipGetLastError());
    if (!W.timed) { h->t_total_ms = ev_ms(W.ev_begin, ev_end); return RSREC_OK; }
    finish_timing(h, W.ev_begin, ev_end, W.hop_ev);
    h->n_hop_launch = (double)W.hop_ev.size();
    if (!rest_is_own_spans) return RSREC_OK;
    h->t_rest_ms = 0;
    for (auto& pr : W.rest_ev) h->t_rest_ms += ev_ms(pr.first, pr.second);
    const double fan = (double)std::count_if(h->nbr.begin(), h->nbr.end(), [](int nbr) { return nbr >= 0; });
    h->n_block_mult = fan * W.chain_launches;
    h->n_atom_steps = (double)h->kk * W.chain_launches;
    return RSREC_OK;
}

// The device memory of a rsrec_kubo_moments call, decided before anything is reserved: 11 work vectors, `lchunk` left vectors, one block of
// right vectors per output operator (`nout`; 1 but for rsrec_kubo_moments_diag_multi), the slices' partial blocks, `nout` moment images of
// the vectors in flight -- the five buffers of d_kubo, in that order.  rsrec_kubo_moments_diag_tensor (`nin` input operators): the right
// recurrences of all inputs advance as nin x nbv chains of one launch, so the work vectors and the right slots are nin times as wide
// (the left slots are not), there are nin x nout sets of moments, and the partial buffer holds one image per set of a contraction group.
// The left matrix is held in chunks of `lchunk` vectors (all of them if they fit: cond_ll x kk x 5184 B is 21 GB for cond_ll = 500
// on 8 000 atoms, 252 GB on 10^5): each chunk continues the left recurrence where the previous one stopped and is contracted
// with ALL right vectors, so the right recurrence (2 of the 3 SpMMs per moment order) is repeated once per chunk.
// Vectors in flight: the vectors of a call are independent (recursion.f90:1104: one pass of the loop each) and one whole-lattice product is
// kk / 8 groups -- 1 000 on 8 000 atoms, half a round of the device's wave slots per spin.  Up to 8 of them advance together as the CHAINS of
// every launch (chain c of a buffer slot lies c vectors behind chain 0, exactly like the sites of a recursion batch); each keeps its own
// left / right matrices and is contracted by itself.  A whole left matrix per vector goes first: vectors are added only while it fits.
struct KuboPlan {
    int cond_ll = 0, n_cu = 0, nout = 1;     // nout: output operators of the call, each with right slots of its own
    int nin = 1, setgroup = 1;               // input operators (sets: nin x nout, input outermost); sets of a vector contracted per k_kubo_gram_diag_sets launch (1: k_kubo_gram_diag)
    bool diag = false, resident = false;     // rsrec_kubo_moments_diag: 18 instead of 324 elements per (n, m); the moments of ALL vectors of the call fit d_kubo[4]
    int nchunk = 0, lchunk = 0, nbv = 0;     // right vectors per contraction; left vectors held at a time; vectors in flight
    int ksteps_total = 0, nbn_max = 0;       // k-steps of 4 rows (the last one may end inside the zero block); column blocks of a full contraction
    size_t velems = 0, sstride = 0, lstride = 0;   // doubles of one vector; between two work vectors / right slots (nin x nbv chains each); between two left slots (nbv chains)
    size_t part_image = 0;                   // double2 of one set's slice partials (diag)
    size_t bytes[5] = {0, 0, 0, 0, 0};       // of the five buffers
    // slices of the row index per contraction: enough wave tasks for a dozen rounds of the device, at least 64 k-steps per task.  diag: one
    // workgroup per task, three of them per CU (158 registers); otherwise one wave per task, eight per CU
    int ksplit_for(int lc) const {
        const long blocks = (long)(diag ? (lc + KD_T - 1) / KD_T : (lc * NB + KG_BLK - 1) / KG_BLK) * nbn_max;
        long ksp = (12L * (diag ? 3 : 8) * n_cu + blocks - 1) / std::max(1L, blocks);
        ksp = std::min<long>({ksp, 64, std::max(1, ksteps_total / 64)});
        return (int)std::max<long>(8, (ksp + 7) / 8 * 8);
    }
    // where the buffers lie (kubo_reserve).  The slots of Lm / Rm ARE the left / right vectors (CI layout = dense row-major (18 kk) x 18
    // matrices side by side), written there by the SpMMs themselves and contracted in place.
    double *work = nullptr, *Lm = nullptr, *Rm = nullptr;
    double2 *part = nullptr, *mu = nullptr;
    enum { PSIREF = 0, Y = 1 /* .. 3: the right recurrence */, L0 = 4, HPS = 6, P1 = 7, P2 = 8, L1 = 9 };   // work vectors (L0, L1: T_{m0-2} r, T_{m0-1} r, the left recurrence across a chunk border)
    double* vec(int v) const { return work + (size_t)v * sstride; }
    double* Lslot(int q) const { return Lm + (size_t)q * lstride; }
    double* Rslot(int j, int q) const { return Rm + ((size_t)j * nchunk + q) * sstride; }      // slot q of output operator j (all inputs' chains)
};

constexpr int KUBO_CHAINS_MAX = 8;           // chains of a whole-lattice launch of the Kubo calls
constexpr int KUBO_SETGROUP_MAX = 3;         // widest k_kubo_gram_diag_sets built
constexpr int KUBO_SETGROUP_DEFAULT = 2;     // what kubo_setgroup = 0 means: pairs measured 0.75 of the per-set contraction at cond_ll = 500, triples (one workgroup per CU) 1.01

int kubo_plan(rsrec_t* h, int nin, int nout, int setgroup, int nvec, int cond_ll, bool diag, KuboPlan& P) {
    const int kk = h->kk;
    P.diag = diag; P.nout = nout; P.nin = nin;
    const int nset = nin * nout;
    P.setgroup = std::max(1, std::min({setgroup, KUBO_SETGROUP_MAX, nset}));
    P.cond_ll = cond_ll; P.n_cu = h->n_cu; P.velems = (size_t)(kk + 1) * BLD;
    P.nchunk = std::min(cond_ll, 64);
    size_t free_b = 0, total_b = 0;
    HIPCK(h, hipMemGetInfo(&free_b, &total_b));
    size_t reusable = 0;
    for (int v = 0; v < 6; ++v) reusable += h->d_vec[v].bytes;
    for (auto& kb : h->d_kubo) reusable += kb.bytes;             // the buffers of the previous call (reused where they are large enough)
    const double budget = 0.9 * (double)(free_b + reusable);
    P.ksteps_total = (int)((NB * (size_t)kk + 3) / 4);
    P.nbn_max = diag ? (P.nchunk + KD_T - 1) / KD_T : (P.nchunk * NB + KG_BLK - 1) / KG_BLK;
    const double mu_bytes = (double)cond_ll * cond_ll * (diag ? NB : BLK) * 16.0;  // one vector's moments
    auto part_bytes = [&](int lc) {
        if (diag) return (double)P.ksplit_for(lc) * ((lc + KD_T - 1) / KD_T) * KD_T * (double)P.nbn_max * KD_T * NB * 16.0;
        return (double)P.ksplit_for(lc) * ((lc * NB + KG_BLK - 1) / KG_BLK) * KG_BLK * (double)P.nbn_max * KG_BLK * 16.0; };
    auto need_for = [&](int lc, int nv) { return (11.0 * nin + lc + (double)nset * P.nchunk) * nv * P.velems * 8 + P.setgroup * part_bytes(lc) + (double)nv * nset * mu_bytes; };
    int lchunk = cond_ll;
    if (h->opt_kubo_lchunk > 0) lchunk = (int)std::min<long>(cond_ll, h->opt_kubo_lchunk);
    int nbv = (int)std::min<long>({(long)nvec, h->opt_kubo_vbatch > 0 ? h->opt_kubo_vbatch : KUBO_CHAINS_MAX, (long)(KUBO_CHAINS_MAX / nin)});   // nin x nbv chains per launch
    while (nbv > 1 && need_for(lchunk, nbv) > budget) --nbv;
    while (lchunk > 1 && need_for(lchunk, nbv) > budget) lchunk = (lchunk + 1) / 2;
    if (need_for(lchunk, nbv) > budget)
        return fail(h, RSREC_ERR_DEVICE, "rsrec_kubo_moments: %.1f GB needed for one left vector at a time on %d atoms, %.1f GB free", need_for(1, 1) * 1e-9, kk, free_b * 1e-9);
    P.lchunk = lchunk; P.nbv = nbv; P.lstride = (size_t)nbv * P.velems; P.sstride = (size_t)nin * P.lstride;
    P.bytes[0] = 11 * P.sstride * 8; P.bytes[1] = (size_t)lchunk * P.lstride * 8; P.bytes[2] = (size_t)nout * P.nchunk * P.sstride * 8;
    // the diagonal moments of the whole call stay on the handle if they fit beside everything else; lchunk and nbv do not depend on it
    P.resident = diag && need_for(lchunk, nbv) + (double)(nvec - nbv) * nset * mu_bytes <= budget;
    P.part_image = (size_t)part_bytes(lchunk) / 16;
    P.bytes[3] = P.setgroup * P.part_image * 16; P.bytes[4] = (size_t)(P.resident ? nvec : nbv) * nset * (size_t)mu_bytes;
    return RSREC_OK;
}

// The five Kubo buffers at the sizes a plan wants.  Buffers that have to grow are given back first; one that is larger than wanted stays.  The
// plans count ALL bytes of the old buffers as free, so a buffer kept oversize (the work vectors of a single-shot call before a moment call)
// can make a hipMalloc fail that the plan allowed: then everything is given back and asked for once more.
int reserve_kubo_buffers(rsrec_t* h, const size_t (&want)[5], const char* who) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        for (int q = 0; q < 5; ++q) if (attempt || h->d_kubo[q].bytes < want[q]) h->d_kubo[q].release();
        bool ok = true;
        for (int q = 0; q < 5 && ok; ++q) ok = h->d_kubo[q].reserve(want[q]) == hipSuccess;
        if (ok) return RSREC_OK;
        (void)hipGetLastError();
    }
    for (auto& kb : h->d_kubo) kb.release();
    return fail(h, RSREC_ERR_DEVICE, "%s: out of device memory (%.0f bytes needed)", who, (double)(want[0] + want[1] + want[2] + want[3] + want[4]));
}

// The plan's buffers: the recursion's work vectors go, and buffers that have to grow are given back first (reserve_kubo_buffers), so that the
// new sizes are asked of the memory the budget counted on.  Block kk of every vector and slot stays the zero block.
int kubo_reserve(rsrec_t* h, KuboPlan& P) {
    for (int v = 0; v < 6; ++v) h->d_vec[v].release();
    XFER(reserve_kubo_buffers(h, P.bytes, "rsrec_kubo_moments"));
    P.work = h->d_kubo[0].as<double>(); P.Lm = h->d_kubo[1].as<double>(); P.Rm = h->d_kubo[2].as<double>();
    P.part = h->d_kubo[3].as<double2>(); P.mu = h->d_kubo[4].as<double2>();
    HIPCK(h, hipMemsetAsync(P.Lm, 0, P.bytes[1], h->stream));
    HIPCK(h, hipMemsetAsync(P.Rm, 0, P.bytes[2], h->stream));
    HIPCK(h, hipMemsetAsync(P.work, 0, P.bytes[0], h->stream));
    return RSREC_OK;
}

struct KuboSeeds { int nseed; const int32_t* atoms; const double* coef; };   // the caller's (nvec, nseed) tables; atom 0 = unused entry

// The used entries of vector iv in the caller's order: 0-based atoms and their coefficients (re, im).  k_seed places them in this order, so
// of several entries on one atom the last one is the coefficient that is placed.
void whole_vector_seeds(const KuboSeeds& S, int iv, std::vector<int>& s0, std::vector<double>& c0) {
    s0.clear(); c0.clear();
    for (int k = 0; k < S.nseed; ++k) {
        const size_t e = (size_t)iv * S.nseed + k;
        if (S.atoms[e] == 0) continue;
        s0.push_back(S.atoms[e] - 1); c0.push_back(S.coef[2 * e]); c0.push_back(S.coef[2 * e + 1]);
    }
}

// r_i of vectors iv0 .. iv0 + nb - 1 as the chains of `vec` (cleared by the caller), in layout L: vec(l,l,seed(k)) = coef(k).  What
// rsrec_kubo_moments and rsrec_chebyshev_lattice (`who`) share; d_seed and d_seedcoef hold nseed entries.
template <class L>
int seed_whole_vectors(rsrec_t* h, const char* who, const KuboSeeds& S, int iv0, int nb, double* vec, size_t velems) {
    std::vector<int> s0; std::vector<double> c0;
    for (int c = 0; c < nb; ++c) {
        whole_vector_seeds(S, iv0 + c, s0, c0);
        if (s0.empty()) return fail(h, RSREC_ERR_ARG, "%s: vector %d has no seed", who, iv0 + c + 1);
        XFER(xfer_h2d(h, h->d_seed.p, s0.data(), s0.size() * 4));
        XFER(xfer_h2d(h, h->d_seedcoef.p, c0.data(), c0.size() * 8));
        k_seed<L><<<1, 64, 0, h->stream>>>(vec + (size_t)c * velems, velems, h->d_seed.as<int>(), h->d_seedcoef.as<double2>(), (int)s0.size());
        HIPCK(h, hipStreamSynchronize(h->stream));                            // the seed tables are reused by the next vector
    }
    return RSREC_OK;
}

// r_i of vectors iv0 .. iv0 + nb - 1 as the chains of PSIREF: psiref(l,l,seed(k)) = coef(k)
int kubo_seed_batch(rsrec_t* h, const KuboPlan& P, const KuboSeeds& S, int iv0, int nb) {
    double* psiref = P.vec(KuboPlan::PSIREF);
    HIPCK(h, hipMemsetAsync(psiref, 0, P.sstride * 8, h->stream));
    return seed_whole_vectors<LayoutCI>(h, "rsrec_kubo_moments", S, iv0, nb, psiref, P.velems);
}

// Left vectors  T_{m-1}(H~) r,  m = m0 .. m0 + lchunk - 1 (recursion.f90:1120-1142), each written by its SpMM into its slot of Lm; the
// recurrence reads the two slots before it -- across a chunk border the copies L0 = T_{m0-2} r, L1 = T_{m0-1} r, saved here for the next chunk
int kubo_left_chunk(WholeLatticeCall& W, const KuboPlan& P, int m0, double a, double b) {
    rsrec_t* h = W.h;
    const int ml = std::min(P.lchunk, P.cond_ll - m0);
    const size_t cpy = ((size_t)W.SD.nchains * P.velems - BLD) * 8;      // the chains of a slot, up to the last one's zero block
    double *l0 = P.vec(KuboPlan::L0), *l1 = P.vec(KuboPlan::L1);
    for (int m = m0; m < m0 + ml; ++m) {
        double* out = P.Lslot(m - m0);
        const double* prev1 = m - 1 >= m0 ? P.Lslot(m - 1 - m0) : l1;
        const double* prev2 = m - 2 >= m0 ? P.Lslot(m - 2 - m0) : (m - 2 == m0 - 1 ? l1 : l0);
        if (m == 0) HIPCK(h, hipMemcpyAsync(out, P.vec(KuboPlan::PSIREF), cpy, hipMemcpyDeviceToDevice, h->stream));
        else if (m == 1) whole_lattice_apply_h(W, prev1, out, cheb_epilogue(true, prev1, nullptr, a, b));
        else whole_lattice_apply_h(W, prev1, out, cheb_epilogue(false, prev1, prev2, a, b));
    }
    if (m0 + ml < P.cond_ll) {                                          // (the slots are about to be reused)
        if (ml >= 2) HIPCK(h, hipMemcpyAsync(l0, P.Lslot(ml - 2), cpy, hipMemcpyDeviceToDevice, h->stream));
        else HIPCK(h, hipMemcpyAsync(l0, l1, cpy, hipMemcpyDeviceToDevice, h->stream));
        HIPCK(h, hipMemcpyAsync(l1, P.Lslot(ml - 1), cpy, hipMemcpyDeviceToDevice, h->stream));
    }
    return RSREC_OK;
}

// Slices of a contraction of nbm x nbn tiles: the multiple of 8 (<= what the partial buffer was sized for, >= 64 k-steps per task) that fills
// whole rounds of the device's `per_cu` task slots per CU best (8 waves: k_kubo_gram; 3 workgroups: k_kubo_gram_diag and
// k_kubo_gram_diag_sets) -- 361 blocks x 24 slices are 4.2 rounds of 2 048 slots (85 % of the last round idle), x 32 are 5.6.  The slice
// partition decides the order of every element's sum, so a set's bits are the same whichever diagonal kernel contracts it.
int kubo_ksplit(const rsrec_t* h, const KuboPlan& P, int per_cu, int nbm, int nbn) {
    int ksplit = 8;
    const long slots = (long)per_cu * h->n_cu, cap = std::min<long>(P.ksplit_for(P.lchunk), std::max(8, P.ksteps_total / 64 / 8 * 8));
    double best = 0.0;
    for (long c = 8; c <= cap; c += 8) {
        const long tasks = (long)nbm * nbn * c, rounds = (tasks + slots - 1) / slots;
        const double eff = (double)tasks / (double)(rounds * slots) * (rounds >= 3 ? 1.0 : 0.9);   // (few rounds: the tail of the slowest wave shows)
        if (eff > best + 1e-9) { best = eff; ksplit = (int)c; }
    }
    return ksplit;
}

// The same for the orbital-diagonal moments alone: per column c the Gram matrix of the chunk's left and the block's right vectors, tiles of
// 16 x 16 vectors x all 18 columns x `ksplit` slices of (k,r), one workgroup each (k_kubo_gram_diag), then k_kubo_gram_diag_reduce.
// Sets s_lo .. s_lo + ns - 1 of the call (set s = input s / nout, output s % nout: the right vectors are the chains of input i in the slots
// of output j) for the `nb` vectors of the batch; ns = 1: k_kubo_gram_diag, 2 or 3: k_kubo_gram_diag_sets, one partial image per set.
// mu_off(s): where the batch's first vector of set s lies in P.mu (resident moments of the whole call; the images of the sets), in vectors.
template <class MuOff>
int kubo_contract_diag(WholeLatticeCall& W, const KuboPlan& P, int nb, int s_lo, int ns, int m0, int n, MuOff&& mu_off) {
    rsrec_t* h = W.h;
    const int nl = n % P.nchunk, n0 = n - nl, nv = nl + 1, mv = std::min(P.lchunk, P.cond_ll - m0);
    const int nbm = (mv + KD_T - 1) / KD_T, nbn = (nv + KD_T - 1) / KD_T;
    const int ksplit = kubo_ksplit(h, P, 3, nbm, nbn);
    if (ns < 1 || ns > P.setgroup || (size_t)ksplit * nbm * KD_T * nbn * KD_T * NB > P.part_image)
        return fail(h, RSREC_ERR_DEVICE, "rsrec_kubo_moments: contraction group outside the planned partial buffer");
    HIPCK(h, hipGetLastError());
    hipEvent_t g0 = next_event(h);
    const unsigned wgs = 8u * (unsigned)((long)nbm * nbn * (ksplit / 8));
    const size_t mu_vec = (size_t)P.cond_ll * P.cond_ll * NB;
    for (int c = 0; c < nb; ++c) {
        const double* L = P.Lm + (size_t)c * P.velems;
        auto right = [&](int s) { return P.Rslot(s % P.nout, 0) + ((size_t)(s / P.nout) * nb + c) * P.velems; };
        if (ns == 1) k_kubo_gram_diag<<<wgs, 256, 0, h->stream>>>(L, P.lstride, mv, right(s_lo), P.sstride, nv, P.ksteps_total, ksplit, P.part, nbm, nbn);
        else if (ns == 2) k_kubo_gram_diag_sets<2><<<wgs, 256, 0, h->stream>>>(L, P.lstride, mv, KuboRights<2>{{right(s_lo), right(s_lo + 1)}}, P.sstride, nv, P.ksteps_total, ksplit, P.part, P.part_image, nbm, nbn);
        else k_kubo_gram_diag_sets<3><<<wgs, 256, 0, h->stream>>>(L, P.lstride, mv, KuboRights<3>{{right(s_lo), right(s_lo + 1), right(s_lo + 2)}}, P.sstride, nv, P.ksteps_total, ksplit, P.part, P.part_image, nbm, nbn);
        for (int g = 0; g < ns; ++g)
            k_kubo_gram_diag_reduce<<<(int)std::min<long>(4096, ((long)mv * nv * NB + 255) / 256), 256, 0, h->stream>>>(P.part + (size_t)g * P.part_image, ksplit, nbm * KD_T, nbn * KD_T, mv, nv, P.mu + (mu_off(s_lo + g) + c) * mu_vec, P.cond_ll, m0, n0);
    }
    W.rest_ev.emplace_back(g0, next_event(h));
    return RSREC_OK;
}

// The block of right vectors of set j that ends with order n (its slots 0 .. n % nchunk of Rm) against the left chunk from m0 on, between its events:
// C[(m,c)][(n,c')] = sum_{k,r} conj(L_m[(k,r)][c]) R_n[(k,r)][c'], blocks of C x `ksplit` slices of (k,r), one wave each (k_kubo_gram), then
// the slices summed in fixed order into mu (k_kubo_gram_reduce).  One contraction per vector of the batch: its matrices are the chain-c
// columns of the slots (leading dimension = a whole slot).
int kubo_contract(WholeLatticeCall& W, const KuboPlan& P, int j, int m0, int n) {
    rsrec_t* h = W.h;
    const int nl = n % P.nchunk, n0 = n - nl, ncols = (nl + 1) * NB, m_rows = std::min(P.lchunk, P.cond_ll - m0) * NB;
    const int nbm = (m_rows + KG_BLK - 1) / KG_BLK, nbn = (ncols + KG_BLK - 1) / KG_BLK;
    const int ksplit = kubo_ksplit(h, P, 8, nbm, nbn);
    HIPCK(h, hipGetLastError());
    hipEvent_t g0 = next_event(h);
    const unsigned wgs = 8u * (unsigned)(((long)nbm * nbn * (ksplit / 8) + 3) / 4);
    const size_t mu_vec = (size_t)P.cond_ll * P.cond_ll * BLK;
    for (int c = 0; c < W.SD.nchains; ++c) {
        k_kubo_gram<<<wgs, 256, 0, h->stream>>>(P.Lm + (size_t)c * P.velems, P.lstride, m_rows, P.Rslot(j, 0) + (size_t)c * P.velems, P.sstride, ncols, P.ksteps_total, ksplit, P.part, nbm, nbn);
        k_kubo_gram_reduce<<<std::min(4096, (m_rows * ncols + 255) / 256), 256, 0, h->stream>>>(P.part, ksplit, nbm * KG_BLK, nbn * KG_BLK, m_rows, ncols, P.mu + (size_t)c * mu_vec, P.cond_ll, m0, n0);
    }
    W.rest_ev.emplace_back(g0, next_event(h));
    return RSREC_OK;
}

// What rsrec_kubo_moments, rsrec_kubo_moments_diag, rsrec_kubo_moments_diag_multi and rsrec_kubo_moments_diag_tensor share: everything but
// the contraction kernels and the shape of the result -- `out`: complex (18,18,cond_ll,cond_ll,nvec) on the host, or with `diag` complex
// (18,cond_ll,cond_ll,nvec,nout,nin), host or device or NULL, and then the moments of the whole call stay in d_kubo[4] if they fit there.
// `nout` output operators v_out(:,:,:,:,j) (the single-response calls: 1, v_a) and `nin` input operators v_in(:,:,:,:,i) (all but the tensor
// call: 1, v_b); set (j, i), input outermost, has the launches and the bits of the single-response call with (v_a, v_b) = (v_out_j, v_in_i):
//   - the left vectors depend on neither operator: one chunk for all sets, nb chains;
//   - the right recurrences T_{n-1}(H~) v_in_i r of all inputs advance as the nin x nb chains of ONE launch (chain i nb + c: vector c of input i);
//   - per order n every output operator is applied once to all those chains, into a right slot of its own (hoh: after one shared h_bulk pass);
//   - every set is contracted against the left chunk, `setgroup` sets of a vector per launch (kubo_contract_diag).
// `tensor`: the entry point with several inputs; only there option kubo_setgroup applies, and the error texts name v_in / vo_in.
int kubo_moments_run(rsrec_t* h, const char* fn, bool diag, bool tensor, int nin, int nout, int nvec, int nseed, const int32_t* seed_atoms, const double* seed_coef,
                     int cond_ll, double a, double b, const double* v_out, const double* vo_out, const double* v_in, const double* vo_in, double* out) {
    XFER(check_ready(h, fn));
    if (nout < 1 || nout > RSREC_KUBO_NOUT_MAX) return fail(h, RSREC_ERR_ARG, "%s: nout=%d is not in 1..%d", fn, nout, RSREC_KUBO_NOUT_MAX);
    if (nin < 1 || nin > RSREC_KUBO_NIN_MAX) return fail(h, RSREC_ERR_ARG, "%s: nin=%d is not in 1..%d", fn, nin, RSREC_KUBO_NIN_MAX);
    if (nin * nout > RSREC_KUBO_NSET_MAX) return fail(h, RSREC_ERR_ARG, "%s: nin*nout=%d sets, at most %d", fn, nin * nout, RSREC_KUBO_NSET_MAX);
    if (nvec < 0 || nseed < 1 || cond_ll < 1 || (diag && cond_ll > RSREC_COND_LL_MAX) || a == 0.0 || !v_out || !v_in || (!diag && !out) || (nvec > 0 && (!seed_atoms || !seed_coef)))
        return fail(h, RSREC_ERR_ARG, "%s: bad argument", fn);
    if (h->hoh && (!vo_out || !vo_in)) return fail(h, RSREC_ERR_ARG, "%s: hoh requires %s and %s", fn, tensor || nout > 1 ? "vo_out" : "vo_a", tensor ? "vo_in" : "vo_b");
    if (!h->s5_built) return fail(h, RSREC_ERR_ARG, "%s: lattice has too many neighbour slots for the SpMM kernel", fn);
    XFER(check_seeds(h, fn, seed_atoms, (size_t)nvec * nseed, 0));
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    if (nvec == 0) return RSREC_OK;
    h->kubo_diag_nvec = h->kubo_diag_ll = 0;                       // (d_kubo[4] is about to be overwritten)
    release_kubo_buffers(h, false, true);                          // (the integrand's buffers; this call's own stay for the next one)
    const size_t op_doubles = 2 * (size_t)BLK * h->hslots * h->ntype;             // one operator of v_out / vo_out / v_in / vo_in
    for (int j = 0; j < nout; ++j) XFER(build_kubo_operator(h, h->kubo_op[j], v_out + op_doubles * j, vo_out ? vo_out + op_doubles * j : nullptr));
    for (int i = 0; i < nin; ++i) XFER(build_kubo_operator(h, h->kubo_op_b[i], v_in + op_doubles * i, vo_in ? vo_in + op_doubles * i : nullptr));
    if (h->hoh && h->nmax > 0) XFER(build_kubo_hbulk(h));
    const int nset = nin * nout;
    const int setgroup = !tensor ? 1 : (h->opt_kubo_setgroup <= 0 ? KUBO_SETGROUP_DEFAULT : (int)std::min<long>(h->opt_kubo_setgroup, KUBO_SETGROUP_MAX));
    KuboPlan P;
    XFER(kubo_plan(h, nin, nout, setgroup, nvec, cond_ll, diag, P));
    XFER(kubo_reserve(h, P));
    HIPCK(h, h->d_seed.reserve((size_t)nseed * 4));
    HIPCK(h, h->d_seedcoef.reserve((size_t)nseed * sizeof(double2)));
    WholeLatticeCall W;
    XFER(whole_lattice_begin(h, W, P.nbv * nin, true));
    W.hps = P.vec(KuboPlan::HPS); W.p1 = P.vec(KuboPlan::P1); W.p2 = P.vec(KuboPlan::P2);
    W.ev_begin = next_event(h);
    const KuboSeeds S{nseed, seed_atoms, seed_coef};
    const size_t mu_vec = 2 * (size_t)(diag ? NB : BLK) * cond_ll * cond_ll;      // doubles of one vector's moments
    const bool out_dev = diag && out && is_device_ptr(out);       // (the full call's mu_nm is host memory, as ever)
    int n_left_chunks = 0;
    for (int iv0 = 0; iv0 < nvec; iv0 += P.nbv) {
        const int nb = std::min(P.nbv, nvec - iv0);                               // vectors of this batch; chains of its launches: nb (left, v_in r) or nin nb (right)
        // where the batch's moments of set s lie in P.mu, in vectors: the layout of the result (set outermost) if the whole call is resident
        auto mu_off = [&](int s) { return P.resident ? (size_t)s * nvec + iv0 : (size_t)s * P.nbv; };
        whole_lattice_batch(W, nb, false);
        XFER(kubo_seed_batch(h, P, S, iv0, nb));
        for (int m0 = 0; m0 < cond_ll; m0 += P.lchunk, ++n_left_chunks) {
            XFER(kubo_left_chunk(W, P, m0, a, b));
            // right vectors  v_a T_{n-1}(H~) v_b r  (:1154-1187), written into the slots of Rm and contracted with the left vectors of
            // this chunk, 64 at a time
            ChebyshevStepper Y{P.vec(KuboPlan::Y), P.vec(KuboPlan::Y + 1), P.vec(KuboPlan::Y + 2)};
            whole_lattice_apply_v_prepare(W, P.vec(KuboPlan::PSIREF));                     // v1 = v0 = v_in_i r into the chains of input i
            for (int i = 0; i < nin; ++i) whole_lattice_apply_v_prepared(W, h->kubo_op_b[i], P.vec(KuboPlan::PSIREF), Y.cur + (size_t)i * nb * P.velems);
            if (nin > 1) whole_lattice_batch(W, nin * nb, false);
            for (int n = 0; n < cond_ll; ++n) {
                Y.step(W, n, a, b);
                whole_lattice_apply_v_prepare(W, Y.cur);
                for (int j = 0; j < nout; ++j) whole_lattice_apply_v_prepared(W, h->kubo_op[j], Y.cur, P.Rslot(j, n % P.nchunk));
                if (n % P.nchunk == P.nchunk - 1 || n == cond_ll - 1) {
                    if (!diag) XFER(kubo_contract(W, P, 0, m0, n));
                    else for (int s = 0; s < nset; s += P.setgroup) XFER(kubo_contract_diag(W, P, nb, s, std::min(P.setgroup, nset - s), m0, n, mu_off));
                }
            }
            if (nin > 1) whole_lattice_batch(W, nb, false);
        }
        HIPCK(h, hipGetLastError());
        for (int s = 0; s < nset && out; ++s) {
            const double* src = reinterpret_cast<const double*>(P.mu) + mu_vec * mu_off(s);
            double* dst = out + mu_vec * ((size_t)s * nvec + iv0);
            if (out_dev) HIPCK(h, hipMemcpyAsync(dst, src, (size_t)nb * mu_vec * 8, hipMemcpyDeviceToDevice, h->stream));
            else XFER(xfer_d2h(h, dst, src, (size_t)nb * mu_vec * 8));
        }
    }
    XFER(whole_lattice_end(h, W, true));
    h->n_kubo_left_chunks = n_left_chunks; h->kubo_lchunk_planned = P.lchunk;
    if (P.resident) { h->kubo_diag_nvec = nvec * nset; h->kubo_diag_ll = cond_ll; }
    return RSREC_OK;
}

// The device memory of a rsrec_kubo_single_shot call, decided before anything is reserved (as kubo_plan does).  Per vector in flight: the ring
// of P + 2 order slots and the ne accumulators of its left and its right chain, and with hoh the two chains' h psi; once per call the ne
// products W_e = v_out_j R_e of the vector whose Grams are formed, and with hoh h_bulk R_e of all columns (shared by the output operators)
// and the V R_e of a launch's chains.  The vector batch shrinks with ne: 2 nbv <= KUBO_CHAINS_MAX chains, fewer if they do not fit.
constexpr int SHOT_ORDERS_DEFAULT = 16;      // what shot_orders = 0 means: the fastest of 1, 2, 4, 8, 16 in every measured configuration
struct ShotPlan {
    int P = 0, R = 0, nbv = 0, ne = 0, G = 0;    // orders per pass, ring slots, vectors in flight, columns, chains of a final V launch (<= 8)
    int ksteps_total = 0, ksplit = 0;
    size_t velems = 0, slot = 0;                 // doubles of a vector; of a ring slot (2 nbv chains)
    size_t nvectors = 0, bytes_work = 0, bytes_part = 0, bytes_out = 0;
    double *ring = nullptr, *acc = nullptr, *w = nullptr, *hps = nullptr, *p1 = nullptr, *p2 = nullptr;
    double2 *part = nullptr, *full = nullptr, *diag = nullptr;
    double* ring_slot(int n) const { return ring + (size_t)(n % R) * slot; }
    double* acc_of(int chain, int e) const { return acc + ((size_t)chain * ne + e) * velems; }
};

int shot_plan(rsrec_t* h, int nvec, int nout, int ne, ShotPlan& P) {
    const int kk = h->kk;
    const bool hoh = h->hoh != 0;
    P.ne = ne; P.G = std::min(ne, KUBO_CHAINS_MAX);
    P.P = h->opt_shot_orders <= 0 ? SHOT_ORDERS_DEFAULT : (int)std::min<long>(h->opt_shot_orders, SHOT_ORDERS_MAX);
    P.R = P.P + 2;
    P.velems = (size_t)(kk + 1) * BLD;
    P.ksteps_total = (int)((NB * (size_t)kk + 3) / 4);
    P.ksplit = shot_ksplit(P.ksteps_total);
    P.bytes_part = (size_t)ne * P.ksplit * BLK * 16;
    P.bytes_out = (size_t)(BLK + NB) * ne * nvec * nout * 16;
    size_t free_b = 0, total_b = 0;
    HIPCK(h, hipMemGetInfo(&free_b, &total_b));
    size_t reusable = 0;
    for (int v = 0; v < 6; ++v) reusable += h->d_vec[v].bytes;
    for (auto& kb : h->d_kubo) reusable += kb.bytes;
    const double budget = 0.9 * (double)(free_b + reusable);
    auto vectors_for = [&](int nv) { return (size_t)nv * (2 * P.R + 2 * ne + (hoh ? 2 : 0)) + ne + (hoh ? std::max(nv, ne) + std::max(nv, P.G) : 0); };
    auto need_for = [&](int nv) { return (double)vectors_for(nv) * P.velems * 8 + (double)P.bytes_part + (double)P.bytes_out; };
    int nbv = (int)std::min<long>({(long)nvec, h->opt_kubo_vbatch > 0 ? h->opt_kubo_vbatch : KUBO_CHAINS_MAX, (long)(KUBO_CHAINS_MAX / 2)});
    while (nbv > 1 && need_for(nbv) > budget) --nbv;
    if (need_for(nbv) > budget)
        return fail(h, RSREC_ERR_DEVICE, "rsrec_kubo_single_shot: %.0f bytes needed for one vector at a time on %d atoms (ne=%d, shot_orders=%d), %.0f bytes free",
                    need_for(1), kk, ne, P.P, (double)free_b);
    P.nbv = nbv; P.slot = (size_t)2 * nbv * P.velems; P.nvectors = vectors_for(nbv); P.bytes_work = P.nvectors * P.velems * 8;
    return RSREC_OK;
}

// The plan's buffers out of the handle's Kubo buffers: d_kubo[0] the work vectors, [3] the slice partials, [4] the results of the whole call;
// the left and right matrices of an earlier moment call go (the budget counted them as free).  Everything is cleared: block kk of every vector
// stays the zero block, and nothing an earlier call left is ever read.
int shot_reserve(rsrec_t* h, ShotPlan& P) {
    const bool hoh = h->hoh != 0;
    const size_t want[5] = {P.bytes_work, 0, 0, P.bytes_part, P.bytes_out};
    for (int v = 0; v < 6; ++v) h->d_vec[v].release();
    h->d_kubo[1].release(); h->d_kubo[2].release();
    XFER(reserve_kubo_buffers(h, want, "rsrec_kubo_single_shot"));
    double* at = h->d_kubo[0].as<double>();
    auto take = [&](size_t nv) { double* p = at; at += nv * P.velems; return p; };
    P.ring = take((size_t)P.R * 2 * P.nbv);
    P.acc = take((size_t)2 * P.nbv * P.ne);
    P.w = take(P.ne);
    if (hoh) { P.hps = take(2 * P.nbv); P.p1 = take(std::max(P.nbv, P.ne)); P.p2 = take(std::max(P.nbv, P.G)); }
    P.part = h->d_kubo[3].as<double2>();
    P.full = h->d_kubo[4].as<double2>();
    P.diag = P.full + P.bytes_out / 16 / (BLK + NB) * BLK;
    HIPCK(h, hipMemsetAsync(h->d_kubo[0].p, 0, P.bytes_work, h->stream));
    return RSREC_OK;
}

// one accumulation pass: orders n0 .. n0 + cnt - 1 of the ring into the accumulators of the launch's chains (the first nb: left)
void shot_accumulate(rsrec_t* h, const ShotPlan& P, int nb, int n0, int cnt, int cond_ll) {
    const size_t total = (size_t)h->kk * BLK, vs = P.velems / 2;
    const double2* ring = reinterpret_cast<const double2*>(P.ring);
    double2* acc = reinterpret_cast<double2*>(P.acc);
    const double2* w = h->d_shot_w.as<double2>();
    auto go = [&](auto kern, int per_wg) {
        const dim3 grid((unsigned)((total + per_wg - 1) / per_wg), (unsigned)(2 * nb));
        kern<<<grid, SHOT_THREADS, 0, h->stream>>>(ring, P.slot / 2, P.R, n0 % P.R, cnt, vs, total, w, nb, n0, cond_ll, P.ne, acc);
    };
    if (cnt <= 1) go(k_shot_accum<1, 4>, SHOT_THREADS * 4);
    else if (cnt <= 2) go(k_shot_accum<2, 4>, SHOT_THREADS * 4);
    else if (cnt <= 4) go(k_shot_accum<4, 4>, SHOT_THREADS * 4);
    else if (cnt <= 8) go(k_shot_accum<8, 2>, SHOT_THREADS * 2);
    else go(k_shot_accum<16, 1>, SHOT_THREADS);
}

// rsrec_kubo_single_shot behind its argument checks.  Per batch of nb vectors: chains 0 .. nb - 1 carry T_n(H~) r, chains nb .. 2 nb - 1
// T_n(H~) v_b r, and both advance in the same cond_ll - 1 launches (twice that with hoh); one launch (hoh: three) forms v_b r.  After every
// P orders and after the last one a pass adds the ring's new orders into the 2 nb ne accumulators.  Final stage, vector by vector: with hoh
// h_bulk R_e of all columns once, then per output operator W_e = v_out_j R_e, up to 8 columns per launch, and the Grams L_e^H W_e of all
// columns in one launch.  SpMM launches of a batch:  cond_ll + nb nout ceil(ne / 8)  (hoh:  2 cond_ll + 1 + nb (1 + 2 nout) ceil(ne / 8)).
int kubo_single_shot_run(rsrec_t* h, const char* fn, int nout, int nvec, int nseed, const int32_t* seed_atoms, const double* seed_coef, int cond_ll, double a,
                         double b, const double* v_out, const double* vo_out, const double* v_b, const double* vo_b, int ne, const double* wl, const double* wr,
                         double* s_full, double* s_diag) {
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    if (nvec == 0) return RSREC_OK;
    h->kubo_diag_nvec = h->kubo_diag_ll = 0;                       // (d_kubo[4] is about to be overwritten)
    release_kubo_buffers(h, false, true);
    const size_t op_doubles = 2 * (size_t)BLK * h->hslots * h->ntype;
    for (int j = 0; j < nout; ++j) XFER(build_kubo_operator(h, h->kubo_op[j], v_out + op_doubles * j, vo_out ? vo_out + op_doubles * j : nullptr));
    XFER(build_kubo_operator(h, h->kubo_op_b[0], v_b, vo_b));
    if (h->hoh && h->nmax > 0) XFER(build_kubo_hbulk(h));
    ShotPlan P;
    XFER(shot_plan(h, nvec, nout, ne, P));
    XFER(shot_reserve(h, P));
    HIPCK(h, h->d_seed.reserve((size_t)nseed * 4));
    HIPCK(h, h->d_seedcoef.reserve((size_t)nseed * sizeof(double2)));
    // the weights as the pass reads them: [side][e][order], side 0 = conj(wl) (the bra side), side 1 = wr
    {
        std::vector<double> wt((size_t)4 * ne * cond_ll);
        for (size_t q = 0; q < (size_t)ne * cond_ll; ++q) {
            wt[2 * q] = wl[2 * q]; wt[2 * q + 1] = -wl[2 * q + 1];
            wt[2 * ((size_t)ne * cond_ll + q)] = wr[2 * q]; wt[2 * ((size_t)ne * cond_ll + q) + 1] = wr[2 * q + 1];
        }
        HIPCK(h, h->d_shot_w.reserve(wt.size() * 8));
        XFER(xfer_h2d(h, h->d_shot_w.p, wt.data(), wt.size() * 8));
    }
    WholeLatticeCall W;
    XFER(whole_lattice_begin(h, W, std::max(2 * P.nbv, P.G), true));
    W.hps = P.hps; W.p2 = P.p2;
    W.ev_begin = next_event(h);
    const KuboSeeds S{nseed, seed_atoms, seed_coef};
    const bool mfma = h->opt_kernels != 1;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> acc_ev, fin_ev;
    const size_t acc_bytes = (size_t)2 * P.nbv * ne * P.velems * 8;
    for (int iv0 = 0; iv0 < nvec; iv0 += P.nbv) {
        const int nb = std::min(P.nbv, nvec - iv0);
        double* r0 = P.ring_slot(0);
        HIPCK(h, hipMemsetAsync(r0, 0, P.slot * 8, h->stream));
        HIPCK(h, hipMemsetAsync(P.acc, 0, acc_bytes, h->stream));
        XFER(seed_whole_vectors<LayoutCI>(h, fn, S, iv0, nb, r0, P.velems));
        whole_lattice_batch(W, nb, false);
        W.p1 = P.p1;
        whole_lattice_apply_v(W, h->kubo_op_b[0], r0, r0 + (size_t)nb * P.velems);          // v_b r into the right chains
        whole_lattice_batch(W, 2 * nb, false);
        for (int n = 0, n0 = 0; n < cond_ll; ++n) {
            if (n >= 1) {
                const double* cur = P.ring_slot(n - 1);
                whole_lattice_apply_h(W, cur, P.ring_slot(n), cheb_epilogue(n == 1, cur, n >= 2 ? P.ring_slot(n - 2) : nullptr, a, b));
            }
            if (n - n0 + 1 == P.P || n == cond_ll - 1) {
                hipEvent_t e0 = next_event(h);
                shot_accumulate(h, P, nb, n0, n - n0 + 1, cond_ll);
                acc_ev.emplace_back(e0, next_event(h));
                n0 = n + 1;
            }
        }
        HIPCK(h, hipGetLastError());
        hipEvent_t f0 = next_event(h);
        for (int c = 0; c < nb; ++c) {
            const double* Rc = P.acc_of(nb + c, 0);
            if (h->hoh)
                for (int e0 = 0; e0 < ne; e0 += P.G) {
                    whole_lattice_batch(W, std::min(P.G, ne - e0), false);
                    W.p1 = P.p1 + (size_t)e0 * P.velems;
                    whole_lattice_apply_v_prepare(W, Rc + (size_t)e0 * P.velems);
                }
            for (int j = 0; j < nout; ++j) {
                for (int e0 = 0; e0 < ne; e0 += P.G) {
                    whole_lattice_batch(W, std::min(P.G, ne - e0), false);
                    W.p1 = h->hoh ? P.p1 + (size_t)e0 * P.velems : nullptr;
                    whole_lattice_apply_v_prepared(W, h->kubo_op[j], Rc + (size_t)e0 * P.velems, P.w + (size_t)e0 * P.velems);
                }
                const dim3 grid((unsigned)P.ksplit, (unsigned)ne);
                if (mfma) k_shot_gram<<<grid, 64, 0, h->stream>>>(P.acc_of(c, 0), P.velems, P.w, P.velems, P.ksteps_total, P.ksplit, P.part);
                else k_shot_gram_valu<<<grid, SHOT_GRAM_VALU_THREADS, 0, h->stream>>>(P.acc_of(c, 0), P.velems, P.w, P.velems, P.ksteps_total, P.ksplit, P.part);
                k_shot_gram_reduce<<<ne, SHOT_GRAM_VALU_THREADS, 0, h->stream>>>(P.part, P.ksplit, ne, iv0 + c, nvec, j, P.full, P.diag);
            }
        }
        fin_ev.emplace_back(f0, next_event(h));
        HIPCK(h, hipGetLastError());
    }
    const size_t nimg = (size_t)ne * nvec * nout;
    auto deliver = [&](double* dst, const double2* src, size_t n) {
        if (!dst) return (int)RSREC_OK;
        if (is_device_ptr(dst)) { HIPCK(h, hipMemcpyAsync(dst, src, n * 16, hipMemcpyDeviceToDevice, h->stream)); return (int)RSREC_OK; }
        return xfer_d2h(h, dst, src, n * 16);
    };
    XFER(deliver(s_full, P.full, nimg * BLK));
    XFER(deliver(s_diag, P.diag, nimg * NB));
    XFER(whole_lattice_end(h, W, true));
    for (auto& pr : acc_ev) h->t_shot_ms[0] += ev_ms(pr.first, pr.second);
    for (auto& pr : fin_ev) h->t_shot_ms[1] += ev_ms(pr.first, pr.second);
    h->t_rest_ms = h->t_shot_ms[0] + h->t_shot_ms[1];
    return RSREC_OK;
}

}  // namespace

// compute_moments_stochastic (recursion.f90:979-1234):  mu(:,:,n,m,i) = sum_k [T_{m-1}(H~) r_i]_k^H [v_a T_{n-1}(H~) v_b r_i]_k,
// H~ = (H - b)/a.  The SpMMs are k_spmm5 over all atoms (blocks outside the reference's growing region are exact zeros); the
// cond_ll x cond_ll moment contraction of a vector is one complex GEMM  L^H R  over the (atom, row) index (k_kubo_gram on the vectors in place).
extern "C" int rsrec_kubo_moments(rsrec_t* h, int nvec, int nseed, const int32_t* seed_atoms, const double* seed_coef, int cond_ll, double a, double b,
                                  const double* v_a, const double* vo_a, const double* v_b, const double* vo_b, double* mu_nm) {
    if (!h) return RSREC_ERR_ARG;
    return kubo_moments_run(h, "rsrec_kubo_moments", false, false, 1, 1, nvec, nseed, seed_atoms, seed_coef, cond_ll, a, b, v_a, vo_a, v_b, vo_b, mu_nm);
}

// The same recurrences, but only the orbital-diagonal moments mu(l,l,n,m,i) are contracted (k_kubo_gram_diag): conductivity.f90:289 and
// :292 are the only reads of mu_nm_stochastic in the reference, and both take (l2, l2, n, m, ntype).
extern "C" int rsrec_kubo_moments_diag(rsrec_t* h, int nvec, int nseed, const int32_t* seed_atoms, const double* seed_coef, int cond_ll, double a, double b,
                                       const double* v_a, const double* vo_a, const double* v_b, const double* vo_b, double* mu_diag) {
    if (!h) return RSREC_ERR_ARG;
    return kubo_moments_run(h, "rsrec_kubo_moments_diag", true, false, 1, 1, nvec, nseed, seed_atoms, seed_coef, cond_ll, a, b, v_a, vo_a, v_b, vo_b, mu_diag);
}

// The diagonal moments of `nout` responses to one applied field: set j is rsrec_kubo_moments_diag with v_a = v_out(:,:,:,:,j).  The left
// vectors, the right recurrence and (hoh) the h_bulk pass of every V product are shared: (2 + nout) cond_ll whole-lattice products
// instead of 3 nout cond_ll.
extern "C" int rsrec_kubo_moments_diag_multi(rsrec_t* h, int nout, int nvec, int nseed, const int32_t* seed_atoms, const double* seed_coef, int cond_ll,
                                             double a, double b, const double* v_out, const double* vo_out, const double* v_b, const double* vo_b,
                                             double* mu_diag) {
    if (!h) return RSREC_ERR_ARG;
    return kubo_moments_run(h, "rsrec_kubo_moments_diag_multi", true, false, 1, nout, nvec, nseed, seed_atoms, seed_coef, cond_ll, a, b, v_out, vo_out, v_b, vo_b, mu_diag);
}

// The diagonal moments of `nout` responses to `nin` applied fields: set (j, i), input outermost, is rsrec_kubo_moments_diag with
// (v_a, v_b) = (v_out(:,:,:,:,j), v_in(:,:,:,:,i)).  Per moment order 1 + nin + nin nout whole-lattice products in 2 + nout launches
// (the inputs' right recurrences are chains of one launch) instead of 3 nin nout, and one staged left tile serves `kubo_setgroup` sets in
// the contraction (k_kubo_gram_diag_sets).
extern "C" int rsrec_kubo_moments_diag_tensor(rsrec_t* h, int nin, int nout, int nvec, int nseed, const int32_t* seed_atoms, const double* seed_coef, int cond_ll,
                                              double a, double b, const double* v_out, const double* vo_out, const double* v_in, const double* vo_in,
                                              double* mu_diag) {
    if (!h) return RSREC_ERR_ARG;
    return kubo_moments_run(h, "rsrec_kubo_moments_diag_tensor", true, true, nin, nout, nvec, nseed, seed_atoms, seed_coef, cond_ll, a, b, v_out, vo_out, v_in, vo_in, mu_diag);
}

// The double sum over the moments of rsrec_kubo_moments at ne weight columns without the moments (kernels_shot.hpp):
//   s(:,:,e,v,j) = sum_{n,m} wl(m,e) wr(n,e) mu_j(:,:,n,m,v),   mu_j = rsrec_kubo_moments with (v_a, v_b) = (v_out_j, v_b)
// 2 (cond_ll - 1) chain steps per vector whatever the cell size, about 2 ne + 2 P + 6 work vectors per vector in flight.
extern "C" int rsrec_kubo_single_shot(rsrec_t* h, int nout, int nvec, int nseed, const int32_t* seed_atoms, const double* seed_coef, int cond_ll, double a, double b,
                                      const double* v_out, const double* vo_out, const double* v_b, const double* vo_b, int ne, const double* wl, const double* wr,
                                      double* s_full, double* s_diag) {
    if (!h) return RSREC_ERR_ARG;
    const char* fn = "rsrec_kubo_single_shot";
    XFER(check_ready(h, fn));
    if (nout < 1 || nout > RSREC_KUBO_NOUT_MAX) return fail(h, RSREC_ERR_ARG, "%s: nout=%d is not in 1..%d", fn, nout, RSREC_KUBO_NOUT_MAX);
    if (ne < 1 || ne > RSREC_KUBO_SHOT_NE_MAX) return fail(h, RSREC_ERR_ARG, "%s: ne=%d is not in 1..%d", fn, ne, RSREC_KUBO_SHOT_NE_MAX);
    if (cond_ll < 1 || cond_ll > RSREC_KUBO_SHOT_LL_MAX) return fail(h, RSREC_ERR_ARG, "%s: cond_ll=%d is not in 1..%d", fn, cond_ll, RSREC_KUBO_SHOT_LL_MAX);
    if (!wl || !wr || !v_out || !v_b) return fail(h, RSREC_ERR_ARG, "%s: wl, wr, v_out and v_b must be given", fn);
    if (!s_full && !s_diag) return fail(h, RSREC_ERR_ARG, "%s: s_full and s_diag are both NULL", fn);
    if (nvec < 0 || nseed < 1 || a == 0.0 || (nvec > 0 && (!seed_atoms || !seed_coef))) return fail(h, RSREC_ERR_ARG, "%s: bad argument", fn);
    if (h->hoh && (!vo_out || !vo_b)) return fail(h, RSREC_ERR_ARG, "%s: hoh requires vo_out and vo_b", fn);
    if (!h->s5_built) return fail(h, RSREC_ERR_ARG, "%s: lattice has too many neighbour slots for the SpMM kernel", fn);
    for (size_t q = 0; q < 2 * (size_t)cond_ll * ne; ++q)
        if (!std::isfinite(wl[q]) || !std::isfinite(wr[q])) return fail(h, RSREC_ERR_ARG, "%s: weight %zu of column %zu is not finite", fn, q / 2 % cond_ll + 1, q / 2 / cond_ll + 1);
    XFER(check_seeds(h, fn, seed_atoms, (size_t)nvec * nseed, 0));
    return kubo_single_shot_run(h, fn, nout, nvec, nseed, seed_atoms, seed_coef, cond_ll, a, b, v_out, vo_out, v_b, vo_b, ne, wl, wr, s_full, s_diag);
}

namespace {

// The energy scale of the conductivity, x = (ene - b) / a, as the reference forms it (conductivity.f90:179-180, :238-241): 2 - 0.3 is default REAL(4)
struct KuboScale {
    double a, b;
    KuboScale(double energy_min, double energy_max) : a((energy_max - energy_min) / (double)(2.0f - 0.3f)), b((energy_max + energy_min) / 2) {}
};

// w_n = g_n weights_n, n = 1 .. L: Lorentz kernel (lambda = 6) x the half weight of n = 1 (conductivity.f90:186-194).  lorentz_kernel forms
// (real(ll) - 1)/real(bign) and 1 - that in single precision (math.f90:1674)
std::vector<double> kubo_kernel_weights(int L) {
    std::vector<double> w(L);
    for (int ll = 1; ll <= L; ++ll) {
        const float r = ((float)ll - 1.0f) / (float)L, t = 1.0f - r;
        w[ll - 1] = std::sinh(6.0 * (double)t) / std::sinh(6.0) * (ll == 1 ? 0.5 : 1.0);
    }
    return w;
}

// Reserve a buffer of the conductivity calls.  The moments' buffers (d_kubo) stay for the next rsrec_kubo_moments call unless this one needs
// their memory; `keep_diag`: the resident diagonal moments (d_kubo[4]) stay even then.
int reserve_beside_kubo(rsrec_t* h, DevBuf& buf, size_t bytes, bool keep_diag) {
    if (!bytes || buf.reserve(bytes) == hipSuccess) return RSREC_OK;
    (void)hipGetLastError();
    if (keep_diag) for (int q = 0; q < 4; ++q) h->d_kubo[q].release();      // (all but the moments)
    else release_kubo_buffers(h, true, false);
    HIPCK(h, buf.reserve(bytes));
    return RSREC_OK;
}

// The conductivity integrand of calculate_gamma_nm + calculate_conductivity_tensor (conductivity.f90:158-268) in factorised form
// (kernels_cond.hpp): integrand(l, i, v) = factor sum_{n,m} Gamma(i,n,m) mu(l,l,n,m,v), no Gamma array.  Vectors one after another:
// the S / D planes of one vector (18 x L x L x 32 B: 144 MB at L = 500) are the largest buffer.
// Shared by rsrec_kubo_integrand (`mu_nm`: the full moments (18,18,L,L,nvec)) and rsrec_kubo_integrand_diag (`diag`; `mu_nm`: the diagonals
// (18,L,L,nvec), or NULL: the resident ones of the last rsrec_kubo_moments_diag call) -- they differ in where k_cond_gather reads.
int kubo_integrand_run(rsrec_t* h, const char* fn, bool diag, int nvec, int cond_ll, const double* mu_nm, int nen, const double* ene, double energy_min,
                       double energy_max, double* integrand) {
    if (nvec < 1 || cond_ll < 1 || cond_ll > RSREC_COND_LL_MAX || nen < 1 || (!diag && !mu_nm) || !ene || !integrand)
        return fail(h, RSREC_ERR_ARG, "%s: bad argument (nvec=%d cond_ll=%d nen=%d)", fn, nvec, cond_ll, nen);
    if (!std::isfinite(energy_min) || !std::isfinite(energy_max) || !(energy_max > energy_min))
        return fail(h, RSREC_ERR_ARG, "%s: energy window [%g, %g] is empty", fn, energy_min, energy_max);
    const bool resident = diag && !mu_nm;
    if (resident) {
        if (!h->kubo_diag_nvec) return fail(h, RSREC_ERR_ARG, "%s: no diagonal moments are resident on the handle (rsrec_kubo_moments_diag first, or pass mu_diag)", fn);
        if (nvec != h->kubo_diag_nvec || cond_ll != h->kubo_diag_ll)
            return fail(h, RSREC_ERR_ARG, "%s: nvec=%d cond_ll=%d asked, the resident moments have nvec=%d cond_ll=%d", fn, nvec, cond_ll, h->kubo_diag_nvec, h->kubo_diag_ll);
        mu_nm = h->d_kubo[4].as<double>();
    }
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    const int L = cond_ll, lk = (L + 3) / 4 * 4, ln = (L + 15) / 16 * 16, ep = (nen + KC_ROWS - 1) / KC_ROWS * KC_ROWS, ntiles = ln / 16;
    // a, b and factor as the reference forms them (:179-180, :254-256)
    const KuboScale sc(energy_min, energy_max);
    const double a = sc.a, b = sc.b, de = energy_max - energy_min;
    const double factor = 16 / (3.14159265358979323846 * (de * de));
    const std::vector<double> w = kubo_kernel_weights(L);
    const bool mu_dev = is_device_ptr(mu_nm), out_dev = is_device_ptr(integrand);
    const size_t per_vec_out = (size_t)NB * nen;
    // buffer 0: tb (lk x ep), ta (ln x ep complex), pre (ep), w (L), ene (nen);  1: S / D planes;  2: partials;  3: staging
    const size_t o_ta = (size_t)lk * ep, o_pre = o_ta + 2 * (size_t)ln * ep, o_w = o_pre + ep, o_ene = o_w + L, n0 = o_ene + nen;
    const size_t mu_elems = (size_t)(diag ? NB : BLK) * L * L;        // complex numbers of one vector's moments as the caller holds them
    const size_t mu_compact = mu_dev ? 0 : (size_t)NB * L * L * 2, n3 = mu_compact + (out_dev ? 0 : 2 * per_vec_out * nvec);
    const size_t want[4] = {n0 * sizeof(double), (size_t)NB * lk * ln * sizeof(double4_t), (size_t)NB * ntiles * ep * sizeof(double2), n3 * sizeof(double)};
    for (int k = 0; k < 4; ++k) XFER(reserve_beside_kubo(h, h->d_cond[k], want[k], resident));      // (resident: the moments being read stay)
    double* T = h->d_cond[0].as<double>();
    XFER(xfer_h2d(h, T + o_w, w.data(), (size_t)L * sizeof(double)));
    XFER(xfer_h2d(h, T + o_ene, ene, (size_t)nen * sizeof(double)));
    hipEvent_t e_begin = next_event(h);
    k_cond_basis<<<(ep + 255) / 256, 256, 0, h->stream>>>(nen, ep, L, lk, ln, T + o_ene, T + o_w, a, b, factor, T, reinterpret_cast<double2*>(T + o_ta), T + o_pre);
    HIPCK(h, hipGetLastError());
    double* stage = h->d_cond[3].as<double>();
    double2* out = out_dev ? reinterpret_cast<double2*>(integrand) : reinterpret_cast<double2*>(stage + mu_compact);
    std::vector<double> dg(mu_dev || diag ? 0 : mu_compact);
    const size_t gelems = (size_t)NB * lk * ln;
    const dim3 cgrid((unsigned)((ep + 4 * KC_ROWS - 1) / (4 * KC_ROWS)), (unsigned)ntiles, NB);
    std::vector<std::pair<hipEvent_t, hipEvent_t>> cev;
    for (int v = 0; v < nvec; ++v) {
        const double2* src;
        int sl, sn;
        if (mu_dev) {
            src = reinterpret_cast<const double2*>(mu_nm) + mu_elems * v;
            sl = diag ? 1 : NB + 1; sn = diag ? NB : BLK;            // the diagonals where they lie: nothing of size 18 x 18 x L x L is copied
        } else {                                                     // host moments: only the 18 diagonals cross the bus
            const double* mv = mu_nm + 2 * mu_elems * v;
            if (!diag) {
                for (size_t nm = 0; nm < (size_t)L * L; ++nm)
                    for (int l = 0; l < NB; ++l) {
                        dg[2 * (nm * NB + l)] = mv[2 * (nm * BLK + (size_t)l * (NB + 1))];
                        dg[2 * (nm * NB + l) + 1] = mv[2 * (nm * BLK + (size_t)l * (NB + 1)) + 1];
                    }
                mv = dg.data();
            }
            XFER(xfer_h2d(h, stage, mv, mu_compact * sizeof(double)));
            src = reinterpret_cast<const double2*>(stage);
            sl = 1; sn = NB;
        }
        k_cond_gather<<<(int)std::min<size_t>(4096, (gelems + 255) / 256), 256, 0, h->stream>>>(src, sl, sn, L, lk, ln, h->d_cond[1].as<double4_t>());
        hipEvent_t c0 = next_event(h);
        k_cond_contract<<<cgrid, 256, 0, h->stream>>>(ep, lk, ln, T, reinterpret_cast<const double2*>(T + o_ta), h->d_cond[1].as<double4_t>(), h->d_cond[2].as<double2>());
        k_cond_reduce<<<(int)((per_vec_out + 255) / 256), 256, 0, h->stream>>>(nen, ep, ntiles, h->d_cond[2].as<double2>(), T + o_pre, out + per_vec_out * v);
        hipEvent_t c1 = next_event(h);
        HIPCK(h, hipGetLastError());
        if (!mu_dev) HIPCK(h, hipStreamSynchronize(h->stream));    // (the staging of the next vector's diagonals is overwritten)
        cev.emplace_back(c0, c1);
    }
    hipEvent_t e_end = next_event(h);
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (!out_dev) XFER(xfer_d2h(h, integrand, out, per_vec_out * nvec * sizeof(double2)));
    h->t_total_ms = ev_ms(e_begin, e_end);
    for (auto& pr : cev) h->t_rest_ms += ev_ms(pr.first, pr.second);      // the contractions (k_cond_contract + k_cond_reduce)
    return RSREC_OK;
}

}  // namespace

extern "C" int rsrec_kubo_integrand(rsrec_t* h, int nvec, int cond_ll, const double* mu_nm, int nen, const double* ene, double energy_min,
                                    double energy_max, double* integrand) {
    if (!h) return RSREC_ERR_ARG;
    return kubo_integrand_run(h, "rsrec_kubo_integrand", false, nvec, cond_ll, mu_nm, nen, ene, energy_min, energy_max, integrand);
}

// The same from the orbital-diagonal moments of rsrec_kubo_moments_diag, handed in or resident on the handle (mu_diag = NULL)
extern "C" int rsrec_kubo_integrand_diag(rsrec_t* h, int nvec, int cond_ll, const double* mu_diag, int nen, const double* ene, double energy_min,
                                         double energy_max, double* integrand) {
    if (!h) return RSREC_ERR_ARG;
    return kubo_integrand_run(h, "rsrec_kubo_integrand_diag", true, nvec, cond_ll, mu_diag, nen, ene, energy_min, energy_max, integrand);
}

namespace {

// The tail of calculate_conductivity_tensor (conductivity.f90:283-372) on the device: the 38 series of every set (k_cond_series) and their
// Fermi-weighted Simpson integrals up to every mesh energy (k_cond_tensor).  Needs no lattice and no Hamiltonian.
int kubo_conductivity_run(rsrec_t* h, int nvec, bool per_vector, int nen, int nv1, const double* ene, double energy_min, double energy_max,
                          double temperature, const double* integrand, double* sigma, double* series) {
    const char* fn = "rsrec_kubo_conductivity";
    if (nvec < 1 || nen < 3 || nv1 < 1 || !ene || !integrand || !sigma)
        return fail(h, RSREC_ERR_ARG, "%s: bad argument (nvec=%d nen=%d nv1=%d)", fn, nvec, nen, nv1);
    if (nen < nv1 + 9) return fail(h, RSREC_ERR_ARG, "%s: nen=%d is below nv1 + 9 = %d, the last point simpson_f weights", fn, nen, nv1 + 9);
    if (!std::isfinite(energy_min) || !std::isfinite(energy_max) || !(energy_max > energy_min))
        return fail(h, RSREC_ERR_ARG, "%s: energy window [%g, %g] is empty", fn, energy_min, energy_max);
    if (!std::isfinite(temperature) || temperature < 0) return fail(h, RSREC_ERR_ARG, "%s: temperature %g is negative or not finite", fn, temperature);
    const size_t nsets = 1 + (per_vector ? (size_t)nvec : 0), ncol = (size_t)CT_ROWS * nsets, n_in = (size_t)2 * NB * nen * nvec, n_out = ncol * nen;
    if (ncol * nen > (size_t)INT32_MAX) return fail(h, RSREC_ERR_ARG, "%s: nvec=%d nen=%d: too many (series, energy) pairs", fn, nvec, nen);
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    const KuboScale sc(energy_min, energy_max);
    const bool in_dev = is_device_ptr(integrand), sig_dev = is_device_ptr(sigma), ser_dev = series && is_device_ptr(series);
    // buffer 0: ene (nen), the series [k][column];  1: staging -- integrand | sigma | series, each only for a caller array on the host
    const size_t o_sig = in_dev ? 0 : n_in, o_ser = o_sig + (sig_dev ? 0 : n_out), n1 = o_ser + (series && !ser_dev ? n_out : 0);
    const bool keep_diag = h->kubo_diag_nvec != 0;                   // resident diagonal moments survive the call
    XFER(reserve_beside_kubo(h, h->d_ctens[0], ((size_t)nen + n_out) * sizeof(double), keep_diag));
    XFER(reserve_beside_kubo(h, h->d_ctens[1], n1 * sizeof(double), keep_diag));
    double* d_ene = h->d_ctens[0].as<double>();
    double* d_sk = d_ene + nen;
    double* stage = h->d_ctens[1].as<double>();
    XFER(xfer_h2d(h, d_ene, ene, (size_t)nen * sizeof(double)));
    if (!in_dev) XFER(xfer_h2d(h, stage, integrand, n_in * sizeof(double)));
    const double2* d_in = reinterpret_cast<const double2*>(in_dev ? integrand : stage);
    double* d_sig = sig_dev ? sigma : stage + o_sig;
    double* d_ser = !series ? nullptr : ser_dev ? series : stage + o_ser;
    const int threads = (int)std::min<size_t>(1024, (ncol + 63) / 64 * 64);
    const dim3 grid((unsigned)nen, (unsigned)((ncol + threads - 1) / threads));
    hipEvent_t e_begin = next_event(h);
    k_cond_series<<<(int)(((size_t)nen * nsets + 255) / 256), 256, 0, h->stream>>>(nen, nvec, (int)nsets, d_in, d_sk, d_ser);
    k_cond_tensor<<<grid, threads, 0, h->stream>>>(nen, nv1, (int)ncol, d_ene, sc.a, sc.b, temperature, d_sk, d_sig);
    hipEvent_t e_end = next_event(h);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (!sig_dev) XFER(xfer_d2h(h, sigma, d_sig, n_out * sizeof(double)));
    if (series && !ser_dev) XFER(xfer_d2h(h, series, d_ser, n_out * sizeof(double)));
    h->t_total_ms = h->t_rest_ms = ev_ms(e_begin, e_end);            // (the call's device work is its two kernels)
    return RSREC_OK;
}

}  // namespace

extern "C" int rsrec_kubo_conductivity(rsrec_t* h, int nvec, int per_vector, int nen, int nv1, const double* ene, double energy_min, double energy_max,
                                       double temperature, const double* integrand, double* sigma, double* series) {
    if (!h) return RSREC_ERR_ARG;
    return kubo_conductivity_run(h, nvec, per_vector != 0, nen, nv1, ene, energy_min, energy_max, temperature, integrand, sigma, series);
}

namespace {

// sigma(omega) from the orbital-diagonal moments (kernels_optical.hpp): per set the tables once, then per chunk of orbitals the moment planes
// (k_opt_gather), stage 1 (k_opt_project), the fused stage 2 (k_opt_fused) and the sum of the tile partials (k_opt_reduce).  The
// projections and partials of a chunk stay below OPT_WORK_BYTES (one orbital at least).  Needs no lattice and no Hamiltonian.
constexpr size_t OPT_WORK_BYTES = (size_t)1 << 30;
int kubo_optical_run(rsrec_t* h, int nset, int cond_ll, const double* mu_diag, int nen, const double* ene, double energy_min, double energy_max, int nw,
                     int nfermi, const double* fermi, double temperature, double* opt) {
    const char* fn = "rsrec_kubo_optical";
    if (nset < 1 || cond_ll < 1 || cond_ll > RSREC_COND_LL_MAX || !ene || !fermi || !opt)
        return fail(h, RSREC_ERR_ARG, "%s: bad argument (nset=%d cond_ll=%d, or a NULL ene, fermi or opt)", fn, nset, cond_ll);
    if (nen < 2 || nen > (1 << 20)) return fail(h, RSREC_ERR_ARG, "%s: nen=%d is outside 2 .. %d", fn, nen, 1 << 20);
    if (nw < 1 || nw > nen - 1) return fail(h, RSREC_ERR_ARG, "%s: nw=%d is outside 1 .. nen - 1 = %d", fn, nw, nen - 1);
    if (nfermi < 1 || nfermi > RSREC_OPT_NFERMI_MAX) return fail(h, RSREC_ERR_ARG, "%s: nfermi=%d is outside 1 .. %d", fn, nfermi, RSREC_OPT_NFERMI_MAX);
    if (!std::isfinite(energy_min) || !std::isfinite(energy_max) || !(energy_max > energy_min))
        return fail(h, RSREC_ERR_ARG, "%s: energy window [%g, %g] is empty", fn, energy_min, energy_max);
    if (!std::isfinite(temperature) || temperature < 0) return fail(h, RSREC_ERR_ARG, "%s: temperature %g is negative or not finite", fn, temperature);
    for (int f = 0; f < nfermi; ++f)
        if (!std::isfinite(fermi[f])) return fail(h, RSREC_ERR_ARG, "%s: Fermi level %d is not finite", fn, f + 1);
    const double step = ene[1] - ene[0];
    if (!std::isfinite(ene[0]) || !std::isfinite(step) || !(step > 0)) return fail(h, RSREC_ERR_ARG, "%s: the mesh does not increase (ene(2) - ene(1) = %g)", fn, step);
    for (int i = 2; i < nen; ++i)
        if (!(std::fabs(ene[i] - ene[0] - i * step) <= 1e-9 * step))
            return fail(h, RSREC_ERR_ARG, "%s: the mesh is not uniform: ene(%d) is %g off ene(1) + %d steps of %g", fn, i + 1, ene[i] - ene[0] - i * step, i, step);
    const bool resident = !mu_diag;
    if (resident) {
        if (!h->kubo_diag_nvec) return fail(h, RSREC_ERR_ARG, "%s: no diagonal moments are resident on the handle (rsrec_kubo_moments_diag first, or pass mu_diag)", fn);
        if (nset != h->kubo_diag_nvec || cond_ll != h->kubo_diag_ll)
            return fail(h, RSREC_ERR_ARG, "%s: nset=%d cond_ll=%d asked, the resident moments have nvec=%d cond_ll=%d", fn, nset, cond_ll, h->kubo_diag_nvec, h->kubo_diag_ll);
        mu_diag = h->d_kubo[4].as<double>();
    }
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    const int L = cond_ll, nf = nfermi, lp = (L + KO_TM - 1) / KO_TM * KO_TM, lk = (L + 3) / 4 * 4, ep = (nen + KO_TI - 1) / KO_TI * KO_TI;
    const int nti = ep / KO_TI, ntj = (nen + KO_TJ - 1) / KO_TJ, nb = ep / KO_FB;
    const KuboScale sc(energy_min, energy_max);
    const double pref = 3.14159265358979323846 / (sc.a * sc.a);
    const std::vector<double> w = kubo_kernel_weights(L);
    const bool mu_dev = is_device_ptr(mu_diag), out_dev = is_device_ptr(opt);
    const size_t mu_set = (size_t)NB * L * L, out_set = (size_t)NB * nw * nf;      // complex numbers of one set
    // the chunk of orbitals: projections + partials of a chunk within OPT_WORK_BYTES
    const size_t pt_l = (size_t)lp * ep * sizeof(double2), part_l = (size_t)nti * ntj * nf * KO_NDIAG * sizeof(double2);
    const int nl_max = (int)std::max<size_t>(1, std::min<size_t>(NB, OPT_WORK_BYTES / (pt_l + part_l)));
    // buffer 0: td (lp x ep), ft (nf x ep), fr (nf x nb complex), w (L), ene (nen), fermi (nf), live (nti x ntj int);  1: moment planes;
    // 2: projections;  3: partials;  4: staging -- a set's diagonals | opt, each only for a caller array on the host
    const size_t o_ft = (size_t)lp * ep, o_fr = o_ft + (size_t)nf * ep, o_w = o_fr + 2 * (size_t)nf * nb, o_ene = o_w + L, o_fermi = o_ene + nen,
                 o_live = o_fermi + nf, n0 = o_live + ((size_t)nti * ntj + 1) / 2;
    const size_t o_out = mu_dev ? 0 : 2 * mu_set, n4 = o_out + (out_dev ? 0 : 2 * out_set * nset);
    const size_t want[5] = {n0 * sizeof(double), (size_t)nl_max * lp * lp * sizeof(double2), nl_max * pt_l, nl_max * part_l, n4 * sizeof(double)};
    const bool keep_diag = h->kubo_diag_nvec != 0;                  // resident diagonal moments survive the call
    for (int k = 0; k < 5; ++k) XFER(reserve_beside_kubo(h, h->d_opt[k], want[k], keep_diag));
    double* T = h->d_opt[0].as<double>();
    XFER(xfer_h2d(h, T + o_w, w.data(), (size_t)L * sizeof(double)));
    XFER(xfer_h2d(h, T + o_ene, ene, (size_t)nen * sizeof(double)));
    XFER(xfer_h2d(h, T + o_fermi, fermi, (size_t)nf * sizeof(double)));
    double2* d_fr = reinterpret_cast<double2*>(T + o_fr);
    int* d_live = reinterpret_cast<int*>(T + o_live);
    double* stage = h->d_opt[4].as<double>();
    double2* out = out_dev ? reinterpret_cast<double2*>(opt) : reinterpret_cast<double2*>(stage + o_out);
    std::vector<std::pair<hipEvent_t, hipEvent_t>> kev;
    hipEvent_t e_begin = next_event(h);
    k_opt_basis<<<(ep + 255) / 256, 256, 0, h->stream>>>(nen, ep, L, lp, nf, T + o_ene, T + o_w, T + o_fermi, sc.a, sc.b, temperature, T, T + o_ft);
    k_opt_fermi_range<<<(nb * nf + 255) / 256, 256, 0, h->stream>>>(nen, ep, nf, T + o_ft, d_fr);
    k_opt_tiles<<<(nti * ntj + 255) / 256, 256, 0, h->stream>>>(nen, ep, nw, nf, nti, ntj, d_fr, d_live);
    HIPCK(h, hipGetLastError());
    kev.emplace_back(e_begin, next_event(h));
    for (int s = 0; s < nset; ++s) {
        const double2* src;
        if (mu_dev) src = reinterpret_cast<const double2*>(mu_diag) + mu_set * s;
        else {
            if (s > 0) HIPCK(h, hipStreamSynchronize(h->stream));    // (the staging of the last set's diagonals is overwritten)
            XFER(xfer_h2d(h, stage, mu_diag + 2 * mu_set * s, 2 * mu_set * sizeof(double)));
            src = reinterpret_cast<const double2*>(stage);
        }
        for (int l0 = 0; l0 < NB; l0 += nl_max) {
            const int nl = std::min(nl_max, NB - l0);
            const size_t gelems = (size_t)nl * lp * lp;
            hipEvent_t c0 = next_event(h);
            k_opt_gather<<<(int)std::min<size_t>(4096, (gelems + 255) / 256), 256, 0, h->stream>>>(src, l0, nl, L, lp, h->d_opt[1].as<double2>());
            k_opt_project<<<dim3((unsigned)((ep + 255) / 256), (unsigned)(lp / KO_TM), (unsigned)nl), 256, 0, h->stream>>>(
                ep, lp, lk, T, h->d_opt[1].as<double2>(), h->d_opt[2].as<double2>());
            k_opt_fused<<<dim3((unsigned)((ntj + 3) / 4), (unsigned)nti, (unsigned)nl), 256, 0, h->stream>>>(
                nen, ep, lp, lk, nw, nf, nti, ntj, T, h->d_opt[2].as<double2>(), T + o_ft, d_live, h->d_opt[3].as<double2>());
            k_opt_reduce<<<(int)(((size_t)nl * nw * nf + 255) / 256), 256, 0, h->stream>>>(nw, nf, nti, ntj, l0, nl, pref, d_live, h->d_opt[3].as<double2>(),
                                                                                            out + out_set * s);
            HIPCK(h, hipGetLastError());
            kev.emplace_back(c0, next_event(h));
        }
    }
    hipEvent_t e_end = next_event(h);
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (!out_dev) XFER(xfer_d2h(h, opt, out, out_set * nset * sizeof(double2)));
    h->t_total_ms = ev_ms(e_begin, e_end);
    for (auto& pr : kev) h->t_rest_ms += ev_ms(pr.first, pr.second);        // the kernels: tables, then gather + the two stages + reduce per chunk
    return RSREC_OK;
}

}  // namespace

extern "C" int rsrec_kubo_optical(rsrec_t* h, int nset, int cond_ll, const double* mu_diag, int nen, const double* ene, double energy_min, double energy_max,
                                  int nw, int nfermi, const double* fermi, double temperature, double* opt) {
    if (!h) return RSREC_ERR_ARG;
    return kubo_optical_run(h, nset, cond_ll, mu_diag, nen, ene, energy_min, energy_max, nw, nfermi, fermi, temperature, opt);
}

// chebyshev_orbital_mod (recursion.f90:2834-3049), the moment part (:2893-3013), device-resident: the seeds are chains advanced together.
// For seed atom s:  psiref = 1 on s;  left = i (Y H~ X - X H~ Y) psiref  (X, Y = alat cr(1,:), alat cr(2,:); H~ = ham_vec_matmul, the
// plain operator also when hoh is set);  v_1 = psiref, v_2 = H~' v_1, v_n = 2 H~' v_{n-1} - v_{n-2}  (H~' = ham_hoh_vec_matmul with hoh);
// mu(:,:,n) = sum_k left_k^H v_n,k.  Every product runs over the whole lattice (the reference sets izero = 1, :2920).
//   mu_orb  complex (18,18,lld): the SUM over the seeds of the call, added in seed order (the reference loops over all kk atoms and
//           divides by kk afterwards, :3006);  mu_seed (optional) complex (18,18,lld,nseeds): every seed's contribution.
extern "C" int rsrec_orbital_moments(rsrec_t* h, int nseeds, const int32_t* seed_atoms, int lld, double a, double b, const double* cr, double alat,
                                     double* mu_orb, double* mu_seed) {
    XFER(check_ready(h, "rsrec_orbital_moments"));
    if (nseeds < 0 || lld < 1 || a == 0.0 || !cr || !mu_orb || (nseeds > 0 && !seed_atoms)) return fail(h, RSREC_ERR_ARG, "rsrec_orbital_moments: bad argument");
    XFER(check_seeds(h, "rsrec_orbital_moments", seed_atoms, (size_t)nseeds, 1));
    if (!h->s5_built) return fail(h, RSREC_ERR_ARG, "rsrec_orbital_moments: lattice has too many neighbour slots for the SpMM kernel");
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    std::fill(mu_orb, mu_orb + 2 * (size_t)BLK * lld, 0.0);
    if (nseeds == 0) return RSREC_OK;
    const int kk = h->kk;
    const bool hoh = h->hoh != 0;
    if (hoh) XFER(build_plain_operator(h));
    const Spmm5Operator& plain = hoh ? h->orb_plain : h->s5_op;
    const size_t velems = (size_t)(kk + 1) * BLD;
    const int nvec = hoh ? 5 : 4;                                  // left, v0, v1, v2 (+ h v of the two-pass product)
    BatchPlan bp;
    XFER(plan_batch(h, nseeds, nvec, velems / 2, bp));
    const int B = bp.batch;
    for (int v = 0; v < nvec; ++v) HIPCK(h, h->d_vec[v].reserve((size_t)B * velems * sizeof(double)));
    XFER(reserve_partials(h, B, 2 * (size_t)B * 256 * 1296 * sizeof(double)));
    HIPCK(h, h->d_seed.reserve((size_t)B * 4));
    HIPCK(h, h->d_seedcoef.reserve((size_t)B * sizeof(double2)));
    HIPCK(h, h->d_scal.reserve((size_t)3 * kk * sizeof(double)));
    HIPCK(h, h->d_zsqr.reserve((size_t)B * lld * BLK * sizeof(double2)));           // the chains' moments
    XFER(xfer_h2d(h, h->d_scal.p, cr, (size_t)3 * kk * sizeof(double)));
    WholeLatticeCall W;
    XFER(whole_lattice_begin(h, W, B, true));
    W.hps = hoh ? h->d_vec[4].as<double>() : nullptr;
    W.ev_begin = next_event(h);
    double2* d_out = h->d_zsqr.as<double2>();
    const size_t ostr = (size_t)lld * BLK;
    std::vector<double> host_out;
    for (int c0 = 0; c0 < nseeds; c0 += B) {
        const int nb = std::min(B, nseeds - c0);
        std::vector<int> s0;
        std::vector<double> one;
        stage_seeds(seed_atoms, nullptr, c0, nb, 1, s0, one);
        XFER(xfer_h2d(h, h->d_seed.p, s0.data(), s0.size() * 4));
        XFER(xfer_h2d(h, h->d_seedcoef.p, one.data(), one.size() * 8));
        whole_lattice_batch(W, nb, true);
        double* left = h->d_vec[0].as<double>();
        ChebyshevStepper V{h->d_vec[1].as<double>(), h->d_vec[2].as<double>(), h->d_vec[3].as<double>()};
        for (int v = 0; v < nvec; ++v) HIPCK(h, hipMemsetAsync(h->d_vec[v].p, 0, (size_t)nb * velems * sizeof(double), h->stream));
        k_seed<LayoutCI><<<nb, 64, 0, h->stream>>>(V.cur, velems, h->d_seed.as<int>(), h->d_seedcoef.as<double2>(), 1);     // v_1 = psiref
        // t = H~ psiref with the plain operator, then the position factors
        whole_lattice_spmm(W, plain, 0, V.cur, left, nullptr, cheb_epilogue(true, V.cur, nullptr, a, b));
        k_orb_left<<<dim3(std::min(kk, 1024), nb), 256, 0, h->stream>>>(kk, velems, h->d_seed.as<int>(), h->d_scal.as<double>(), alat, reinterpret_cast<double2*>(left));
        const dim3 grid_mf(std::max(1, std::min(mfma_workgroups_per_chain(h, nb), (W.CV.ostride / GROUP + MF_WAVES - 1) / MF_WAVES)), nb);
        const dim3 gl = level_grid(h, grid_mf, 0);
        for (int n = 0; n < lld; ++n) {
            V.step(W, n, a, b);
            k_mfma_adot<<<gl, MF_WAVES * 64, 0, h->stream>>>(W.CV, 0, kk, left, V.cur, h->d_partial.as<double>());
            int n2 = gl.x;
            const double* p2 = presum(h, h->d_partial.as<double>(), nb, n2, 1296);
            k_reduce_gram_out<<<nb, 1024, 0, h->stream>>>(p2, n2, d_out + (size_t)n * BLK, ostr, 1);
        }
        HIPCK(h, hipGetLastError());
        host_out.resize((size_t)nb * ostr * 2);
        XFER(xfer_d2h(h, host_out.data(), d_out, host_out.size() * sizeof(double)));
        for (int q = 0; q < nb; ++q) {                                // seed order, like the reference's loop (:2893)
            const double* src = host_out.data() + (size_t)q * ostr * 2;
            for (size_t e = 0; e < ostr * 2; ++e) mu_orb[e] += src[e];
            if (mu_seed) memcpy(mu_seed + (size_t)(c0 + q) * ostr * 2, src, ostr * 2 * sizeof(double));
        }
    }
    XFER(whole_lattice_end(h, W));
    drop_resident(h);
    return RSREC_OK;
}

// ham_vec_matmul / ham_hoh_vec_matmul (recursion.f90:913 / :785): psi_out = (H psi_in - b psi_in) / a on whole vectors
// psi(18,18,kk) in the reference's layout (host arrays); with vel = 1: velo_vec_matmul / velo_hoh_vec_matmul (:587 / :656) with
// the operator blocks v_op (and vo_op with hoh), no scaling.
extern "C" int rsrec_apply_operator(rsrec_t* h, int vel, const double* v_op, const double* vo_op, const double* psi_in, double* psi_out, double a, double b) {
    XFER(check_ready(h, "rsrec_apply_operator"));
    if (!psi_in || !psi_out || (vel != 1 && a == 0.0) || (vel == 1 && (!v_op || (h->hoh && !vo_op))) || vel < 0 || vel > 2) return fail(h, RSREC_ERR_ARG, "rsrec_apply_operator: bad argument");
    if (!h->s5_built) return fail(h, RSREC_ERR_ARG, "rsrec_apply_operator: lattice has too many neighbour slots for the SpMM kernel");
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    const int kk = h->kk;
    const size_t velems = (size_t)(kk + 1) * BLD, nd = (size_t)kk * BLD;
    if (vel == 1) { XFER(build_kubo_operator(h, h->kubo_op[0], v_op, vo_op)); if (h->hoh && h->nmax > 0) XFER(build_kubo_hbulk(h)); }
    if (vel == 2 && h->hoh) XFER(build_plain_operator(h));                              // ham_vec_matmul under hoh: the plain operator (recursion.f90:913)
    for (int v = 0; v < 6; ++v) HIPCK(h, h->d_vec[v].reserve(velems * 8));
    for (int v = 0; v < 6; ++v) HIPCK(h, hipMemsetAsync(h->d_vec[v].p, 0, velems * 8, h->stream));
    WholeLatticeCall W;
    XFER(whole_lattice_begin(h, W, 1, false));
    double* in = h->d_vec[0].as<double>(); double* out = h->d_vec[1].as<double>(); double* tmp = h->d_vec[2].as<double>();
    W.hps = h->d_vec[3].as<double>(); W.p1 = h->d_vec[4].as<double>(); W.p2 = h->d_vec[5].as<double>();
    XFER(xfer_h2d(h, tmp, psi_in, nd * 8));
    W.ev_begin = next_event(h);
    k_block_transpose<true><<<std::min(kk, 2048), 384, 0, h->stream>>>(kk, reinterpret_cast<const double2*>(tmp), reinterpret_cast<double2*>(in));
    if (vel == 1) whole_lattice_apply_v(W, h->kubo_op[0], in, out);
    else {
        if (vel == 2 && h->hoh) whole_lattice_spmm(W, h->orb_plain, 0, in, tmp, nullptr);
        else whole_lattice_apply_h(W, in, tmp);
        k_cheb_combine<true><<<(int)std::min<size_t>(4096, (nd + 255) / 256), 256, 0, h->stream>>>(nd, tmp, in, nullptr, out, a, b);
    }
    k_block_transpose<false><<<std::min(kk, 2048), 384, 0, h->stream>>>(kk, reinterpret_cast<const double2*>(out), reinterpret_cast<double2*>(tmp));
    XFER(whole_lattice_end(h, W));                        // (the span ends before the download)
    XFER(xfer_d2h(h, psi_out, tmp, nd * 8));
    return RSREC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Chebyshev moments from whole-lattice seeds (kernels_lattice.hpp): the Kubo calls' left recurrence -- WholeLatticeCall + ChebyshevStepper on
// vectors seeded like theirs -- and behind the seed and every step the projection of the vector on the seed, group by group
namespace {

struct LatticeCall {
    int nchains, lld, ngroup;
    KuboSeeds S;
    const int32_t* group;
    double a, b;
    double* m_g;
};

// The lists of chains c0 .. c0 + nb - 1 as LatticeLists takes them: per chain the seeded atoms of groups 1 .. ngroup sorted by (group, atom)
// with the conjugate of the coefficient k_seed leaves there (the last entry on an atom), the groups' segments and partial slots, and the
// divergence bound 1000 max(1, sum |c|^2) over the placed coefficients, added in atom order.
struct LatticeBatchLists { std::vector<int> list, seg_off, split_off; std::vector<double> weight, bound; int pstride = 1; };
void lattice_lists(const rsrec_t* h, const LatticeCall& A, int c0, int nb, LatticeBatchLists& T) {
    const int kk = h->kk, ng = A.ngroup;
    T.list.assign((size_t)nb * kk, 0); T.weight.assign((size_t)2 * nb * kk, 0.0);
    T.seg_off.assign((size_t)nb * (ng + 1), 0); T.split_off.assign((size_t)nb * (ng + 1), 0); T.bound.assign(nb, 0.0);
    T.pstride = 1;
    std::vector<int> s0, placed(kk), fill(ng);
    std::vector<double> cf;
    for (int c = 0; c < nb; ++c) {
        whole_vector_seeds(A.S, c0 + c, s0, cf);
        std::fill(placed.begin(), placed.end(), -1);
        for (size_t k = 0; k < s0.size(); ++k) placed[s0[k]] = (int)k;
        int *goff = T.seg_off.data() + (size_t)c * (ng + 1), *soff = T.split_off.data() + (size_t)c * (ng + 1);
        double norm2 = 0.0;
        for (int j = 0; j < kk; ++j) {
            if (placed[j] < 0) continue;
            norm2 += cf[2 * placed[j]] * cf[2 * placed[j]] + cf[2 * placed[j] + 1] * cf[2 * placed[j] + 1];
            const int g = A.group ? A.group[j] : 1;
            if (g > 0) goff[g] += 1;
        }
        for (int g = 0; g < ng; ++g) {
            soff[g + 1] = soff[g] + lattice_splits(goff[g + 1]);
            fill[g] = goff[g];
            goff[g + 1] += goff[g];
        }
        for (int j = 0; j < kk; ++j) {
            const int g = A.group ? A.group[j] : 1;
            if (placed[j] < 0 || g <= 0) continue;
            const size_t pos = (size_t)c * kk + fill[g - 1]++;
            T.list[pos] = j; T.weight[2 * pos] = cf[2 * placed[j]]; T.weight[2 * pos + 1] = -cf[2 * placed[j] + 1];
        }
        T.pstride = std::max(T.pstride, soff[ng]);
        T.bound[c] = 1000.0 * std::max(1.0, norm2);
    }
}

// The step of ChebyshevStepper with the VALU set's k_apply on LayoutCM vectors, over the list of all atoms (level 0 of the one region):
// Y.cur = (H old - b old)/a [* 2 - spare]; with hoh h old goes into `tmp` first.  k_apply also writes its Gram partials (d_partial), which
// nothing reads here.  Every launch between its own events, as whole_lattice_spmm's.
void lattice_step_valu(WholeLatticeCall& W, ChebyshevStepper& Y, const DevProblem& P, int nblk, int n, double a, double b, double* tmp) {
    if (n == 0) return;
    rsrec_t* h = W.h;
    Y.rotate(n);
    const bool first = n == 1;
    const dim3 grid(nblk, W.SD.nchains);
    ApplyArgs G{};
    G.partial = h->d_partial.as<double2>(); G.a = a; G.b = b; G.in = Y.old; G.cur = Y.old; G.v0 = first ? Y.old : Y.spare; G.out = Y.cur; G.level = 0;
    auto timed = [&](auto&& launch) {
        hipEvent_t e0 = next_event(h);
        launch();
        W.hop_ev.emplace_back(e0, next_event(h));
        W.chain_launches += W.SD.nchains;
    };
    if (!h->hoh) {
        timed([&] { if (first) k_apply<AM_CHEB1, LayoutCM><<<grid, NTHREADS, 0, h->stream>>>(P, W.CV, G); else k_apply<AM_CHEBN, LayoutCM><<<grid, NTHREADS, 0, h->stream>>>(P, W.CV, G); });
        return;
    }
    G.out = tmp;
    timed([&] { k_apply<AM_STORE, LayoutCM><<<grid, NTHREADS, 0, h->stream>>>(P, W.CV, G); });
    G.in = tmp; G.v1 = tmp; G.out = Y.cur;
    timed([&] { if (first) k_apply<AM_HOH_CHEB1, LayoutCM><<<grid, NTHREADS, 0, h->stream>>>(P, W.CV, G); else k_apply<AM_HOH_CHEBN, LayoutCM><<<grid, NTHREADS, 0, h->stream>>>(P, W.CV, G); });
}

// Matrix-core set: k_spmm5 on CI vectors; VALU set: k_apply on LayoutCM vectors.  Work vectors 0 .. 2: the recurrence; 3 (hoh): h psi.
template <bool MFMA>
int run_lattice(rsrec_t* h, const char* who, const LatticeCall& A) {
    using L = typename std::conditional<MFMA, LayoutCI, LayoutCM>::type;
    const bool hoh = h->hoh != 0;
    const int kk = h->kk, ng = A.ngroup, napply = 2 * A.lld + 1, nmom = 2 * A.lld + 2, nvec = hoh ? 4 : 3;
    const size_t velems = (size_t)(kk + 1) * BLD, mstride = (size_t)nmom * BLK, nimg = (size_t)A.nchains * ng;
    const size_t pmax = (size_t)kk / LATTICE_SPLIT_ATOMS + ng + 1;                // partial slots a chain can need
    // the resident image first, the batch is planned from what is left (see run_chebyshev)
    drop_resident(h);
    release_kubo_buffers(h, true, true);
    HIPCK(h, h->d_mu.reserve(nimg * mstride * sizeof(double2)));
    size_t free_b = 0, total_b = 0, reusable = h->d_lat_tab.bytes + h->d_lat_w.bytes + h->d_lat_part.bytes + (MFMA ? 0 : h->d_partial.bytes + h->d_partial2.bytes);
    HIPCK(h, hipMemGetInfo(&free_b, &total_b));
    for (int v = 0; v < nvec; ++v) reusable += h->d_vec[v].bytes;
    const double per_chain = (double)nvec * velems * 8 + (double)kk * 20 + (double)pmax * BLK * 16 + (MFMA ? 0.0 : 3.0 * 256 * 2 * 1296 * 8) + 4096;
    const double budget = 0.85 * (double)(free_b + reusable);
    int nbv = (int)std::min<long>(A.nchains, h->opt_lattice_vbatch > 0 ? std::min<long>(h->opt_lattice_vbatch, 64) : KUBO_CHAINS_MAX);
    while (nbv > 1 && per_chain * nbv > budget) --nbv;
    if (per_chain * nbv > budget) return fail(h, RSREC_ERR_DEVICE, "%s: %.1f GB needed for one chain on %d atoms, %.1f GB free", who, per_chain * 1e-9, kk, free_b * 1e-9);
    for (int v = 0; v < nvec; ++v) HIPCK(h, h->d_vec[v].reserve((size_t)nbv * velems * sizeof(double)));
    if (!MFMA) XFER(reserve_partials(h, nbv, (size_t)nbv * 256 * 2 * 1296 * sizeof(double)));
    const int nblk = (int)std::max<long>(1, std::min<long>({h->opt_nblk > 0 ? h->opt_nblk : std::max<long>(2048 / nbv, 16), 256, (kk + TILE_ATOMS - 1) / TILE_ATOMS}));
    HIPCK(h, h->d_status.reserve(64));
    HIPCK(h, hipMemsetAsync(h->d_status.p, 0, 64, h->stream));
    HIPCK(h, h->d_seed.reserve((size_t)A.S.nseed * 4));
    HIPCK(h, h->d_seedcoef.reserve((size_t)A.S.nseed * sizeof(double2)));
    const size_t n_list = (size_t)nbv * kk, n_off = (size_t)nbv * (ng + 1);
    HIPCK(h, h->d_lat_tab.reserve((n_list + 2 * n_off) * sizeof(int)));
    HIPCK(h, h->d_lat_w.reserve(n_list * sizeof(double2) + (size_t)nbv * sizeof(double)));
    HIPCK(h, h->d_lat_part.reserve((size_t)nbv * pmax * BLK * sizeof(double2)));
    int *d_list = h->d_lat_tab.as<int>(), *d_seg = d_list + n_list, *d_split = d_seg + n_off;
    double2* d_w = h->d_lat_w.as<double2>();
    double* d_bound = reinterpret_cast<double*>(d_w + n_list);
    double2* partial = h->d_lat_part.as<double2>();
    double2* mu = h->d_mu.as<double2>();
    WholeLatticeCall W;
    XFER(whole_lattice_begin(h, W, nbv, true, MFMA));
    W.hps = hoh ? h->d_vec[3].as<double>() : nullptr;
    const DevProblem P = make_problem(h);
    W.ev_begin = next_event(h);
    LatticeBatchLists T;
    for (int c0 = 0; c0 < A.nchains; c0 += nbv) {
        const int nb = std::min(nbv, A.nchains - c0);
        whole_lattice_batch(W, nb, false);
        lattice_lists(h, A, c0, nb, T);
        if ((size_t)T.pstride > pmax) return fail(h, RSREC_ERR_DEVICE, "%s: split partials outside the planned buffer", who);
        XFER(xfer_h2d(h, d_list, T.list.data(), (size_t)nb * kk * sizeof(int)));
        XFER(xfer_h2d(h, d_seg, T.seg_off.data(), (size_t)nb * (ng + 1) * sizeof(int)));
        XFER(xfer_h2d(h, d_split, T.split_off.data(), (size_t)nb * (ng + 1) * sizeof(int)));
        XFER(xfer_h2d(h, d_w, T.weight.data(), (size_t)nb * kk * sizeof(double2)));
        XFER(xfer_h2d(h, d_bound, T.bound.data(), (size_t)nb * sizeof(double)));
        const LatticeLists LL{d_list, d_w, d_seg, d_split, kk, ng, T.pstride};
        for (int v = 0; v < nvec; ++v) HIPCK(h, hipMemsetAsync(h->d_vec[v].p, 0, (size_t)nb * velems * sizeof(double), h->stream));
        ChebyshevStepper Y{h->d_vec[0].as<double>(), h->d_vec[1].as<double>(), h->d_vec[2].as<double>()};
        XFER(seed_whole_vectors<L>(h, who, A.S, c0, nb, Y.cur, velems));
        for (int n = 0; n <= napply; ++n) {
            if (MFMA) Y.step(W, n, A.a, A.b);
            else lattice_step_valu(W, Y, P, nblk, n, A.a, A.b, h->d_vec[3].as<double>());
            // moment n + 1 of the batch's images: the projection of the vector of order n
            hipEvent_t e0 = next_event(h);
            k_lattice_project<<<dim3(T.pstride, nb), LATTICE_THREADS, 0, h->stream>>>(LL, Y.cur, velems, partial);
            k_lattice_reduce<L><<<dim3(ng, nb, LATTICE_RWG), 64, 0, h->stream>>>(LL, partial, c0, n, nmom, mu);
            k_lattice_diverge<<<nb, LATTICE_THREADS, 0, h->stream>>>(mu, c0, n, nmom, ng, d_bound, h->d_status.as<int>());
            W.rest_ev.emplace_back(e0, next_event(h));
        }
        HIPCK(h, hipGetLastError());
    }
    if (A.m_g) {
        if (is_device_ptr(A.m_g)) HIPCK(h, hipMemcpyAsync(A.m_g, mu, nimg * mstride * sizeof(double2), hipMemcpyDeviceToDevice, h->stream));
        else XFER(xfer_d2h(h, A.m_g, mu, nimg * mstride * sizeof(double2)));
    }
    XFER(whole_lattice_end(h, W, true));
    XFER(finish_status(h));
    h->res_kind = 2; h->res_n = (int)nimg; h->res_lld = A.lld; h->res_seeded = false;   // what an rsrec_chebyshev call of nchains * ngroup sites leaves
    return RSREC_OK;
}

}  // namespace

extern "C" int rsrec_chebyshev_lattice(rsrec_t* h, int nchains, int nseed, const int32_t* seed_atoms, const double* seed_coef, int lld, double a, double b,
                                       int ngroup, const int32_t* group, double* m_g) {
    const char* who = "rsrec_chebyshev_lattice";
    int rc = check_ready(h, who);
    if (rc) return rc;
    if (nchains < 0 || lld < 1 || a == 0.0) return fail(h, RSREC_ERR_ARG, "%s: nchains < 0, lld < 1 or a == 0", who);
    if (nseed < 1 || nseed > h->kk) return fail(h, RSREC_ERR_ARG, "%s: nseed = %d outside 1..%d", who, nseed, h->kk);
    if (ngroup < 1 || ngroup > RSREC_LATTICE_NGROUP_MAX) return fail(h, RSREC_ERR_ARG, "%s: ngroup = %d outside 1..%d", who, ngroup, RSREC_LATTICE_NGROUP_MAX);
    if (nchains > 0 && (!seed_atoms || !seed_coef)) return fail(h, RSREC_ERR_ARG, "%s: NULL seed_atoms or seed_coef", who);
    if (!group && ngroup != 1) return fail(h, RSREC_ERR_ARG, "%s: ngroup = %d needs a group array", who, ngroup);
    if (group)
        for (int j = 0; j < h->kk; ++j)
            if (group[j] < 0 || group[j] > ngroup) return fail(h, RSREC_ERR_ARG, "%s: group(%d) = %d outside 0..%d", who, j + 1, group[j], ngroup);
    XFER(check_seeds(h, who, seed_atoms, (size_t)nchains * nseed, 0));
    for (int c = 0; c < nchains; ++c)
        if (std::all_of(seed_atoms + (size_t)c * nseed, seed_atoms + (size_t)(c + 1) * nseed, [](int32_t s) { return s == 0; }))
            return fail(h, RSREC_ERR_ARG, "%s: vector %d has no seed", who, c + 1);
    if ((size_t)nchains * ngroup > (size_t)INT32_MAX) return fail(h, RSREC_ERR_ARG, "%s: nchains * ngroup exceeds the index range", who);
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    if (nchains == 0) return RSREC_OK;
    const LatticeCall A{nchains, lld, ngroup, KuboSeeds{nseed, seed_atoms, seed_coef}, group, a, b, m_g};
    return matrix_core_set(h) ? run_lattice<true>(h, who, A) : run_lattice<false>(h, who, A);
}

// ------------------------------------------------------------------------------------------------------------------
// Per-atom blocks of ne functions of H from whole-lattice seeds (kernels_sitemap.hpp): the vectors of rsrec_chebyshev_lattice on the ring of
// rsrec_kubo_single_shot, folded over the vectors before the weights are applied, into ne accumulators shared by all vectors of the call
namespace {

constexpr int SITE_ORDERS_DEFAULT = 2, SITE_VTILE_DEFAULT = 8;   // what sitemap_orders = 0 / sitemap_vtile = 0 mean: <8,2>, the fastest call or within 0.02 % of it in 7 of the 9 measured configurations, the four shapes within 1.2 %
constexpr int SITE_STAGE_ATOMS = 512;                            // atoms per slice of a host output: the staging buffer does not grow with kk

struct SiteCall {
    int nvec, lld, ne;
    KuboSeeds S;
    double a, b;
    const double* w;
    double *d_full, *d_diag, *cnorm;
};

// The device memory of a call, decided before anything is reserved.  Per vector in flight: the ring of PT + 2 order slots, with hoh h psi,
// and its coefficient table; once per call the ne accumulators and the staging slice of a host output.
struct SitePlan {
    int VT = 0, PT = 0, R = 0, nbv = 0, ne = 0;
    size_t velems = 0, slot = 0, dstride = 0;      // doubles of a vector; of a ring slot (nbv vectors); complex elements of an accumulator
    size_t bytes_work = 0, bytes_acc = 0, bytes_stage = 0;
    double *ring = nullptr, *hps = nullptr;
    double2 *acc = nullptr, *stage_full = nullptr, *stage_diag = nullptr;
    double* ring_slot(int n) const { return ring + (size_t)(n % R) * slot; }
};

// VT and PT from the options: a value the caller set stays and the other follows it to VT PT = 16 (VT <= 8); of two set values VT gives way
void site_tile_shape(const rsrec_t* h, int& VT, int& PT) {
    auto pow2_floor = [](long v, int hi) { int q = 1; while (2 * q <= v && 2 * q <= hi) q *= 2; return q; };
    VT = h->opt_sitemap_vtile > 0 ? pow2_floor(h->opt_sitemap_vtile, SITE_VTILE_MAX) : SITE_VTILE_DEFAULT;
    PT = h->opt_sitemap_orders > 0 ? pow2_floor(h->opt_sitemap_orders, SITE_ORDERS_MAX) : SITE_ORDERS_DEFAULT;
    if (h->opt_sitemap_vtile > 0 && h->opt_sitemap_orders <= 0) PT = SITE_LOADS_MAX / VT;                    // (the 16 loads stay in flight)
    else if (h->opt_sitemap_orders > 0 && h->opt_sitemap_vtile <= 0) VT = std::min(SITE_VTILE_MAX, SITE_LOADS_MAX / PT);
    else VT = std::min(VT, SITE_LOADS_MAX / PT);
}

int site_plan(rsrec_t* h, const char* who, const SiteCall& A, bool stage, SitePlan& P) {
    const int kk = h->kk;
    const bool hoh = h->hoh != 0;
    site_tile_shape(h, P.VT, P.PT);
    P.R = P.PT + 2; P.ne = A.ne;
    P.velems = (size_t)(kk + 1) * BLD;
    P.dstride = (size_t)kk * BLK;
    P.bytes_acc = (size_t)A.ne * P.dstride * sizeof(double2);
    P.bytes_stage = stage ? (size_t)std::min(kk, SITE_STAGE_ATOMS) * A.ne * (BLK + NB) * sizeof(double2) : 0;
    size_t free_b = 0, total_b = 0;
    HIPCK(h, hipMemGetInfo(&free_b, &total_b));
    size_t reusable = h->d_site_coef.bytes;
    for (int v = 0; v < 6; ++v) reusable += h->d_vec[v].bytes;
    for (auto& kb : h->d_kubo) reusable += kb.bytes;
    const double budget = 0.9 * (double)(free_b + reusable);
    auto need_for = [&](int nv) { return (double)nv * ((P.R + (hoh ? 1 : 0)) * (double)P.velems * 8 + (double)kk * 16) + (double)P.bytes_acc + (double)P.bytes_stage; };
    int nbv = (int)std::min<long>({(long)A.nvec, h->opt_kubo_vbatch > 0 ? h->opt_kubo_vbatch : KUBO_CHAINS_MAX, (long)KUBO_CHAINS_MAX});
    while (nbv > 1 && need_for(nbv) > budget) --nbv;
    if (need_for(nbv) > budget)
        return fail(h, RSREC_ERR_DEVICE, "%s: %.0f bytes needed for one vector at a time on %d atoms (ne=%d, sitemap_orders=%d), %.0f bytes free", who, need_for(1), kk,
                    A.ne, P.PT, (double)free_b);
    P.nbv = nbv; P.slot = (size_t)nbv * P.velems;
    P.bytes_work = (size_t)(P.R + (hoh ? 1 : 0)) * P.slot * 8;
    return RSREC_OK;
}

// The plan's buffers out of the handle's Kubo buffers: d_kubo[0] the ring (and h psi), [3] the accumulators, [4] the staging slice.  The ring is
// cleared (block kk of every vector stays the zero block) and so are the accumulators: once per call, they persist across the batches.
int site_reserve(rsrec_t* h, const char* who, SitePlan& P) {
    const size_t want[5] = {P.bytes_work, 0, 0, P.bytes_acc, P.bytes_stage};
    for (int v = 0; v < 6; ++v) h->d_vec[v].release();
    h->d_kubo[1].release(); h->d_kubo[2].release();
    XFER(reserve_kubo_buffers(h, want, who));
    P.ring = h->d_kubo[0].as<double>();
    P.hps = h->hoh ? P.ring + (size_t)P.R * P.slot : nullptr;
    P.acc = h->d_kubo[3].as<double2>();
    P.stage_full = h->d_kubo[4].as<double2>();
    P.stage_diag = P.stage_full ? P.stage_full + P.bytes_stage / sizeof(double2) / (BLK + NB) * BLK : nullptr;
    HIPCK(h, hipMemsetAsync(h->d_kubo[0].p, 0, P.bytes_work, h->stream));
    HIPCK(h, hipMemsetAsync(h->d_kubo[3].p, 0, P.bytes_acc, h->stream));
    return RSREC_OK;
}

// one accumulation pass of one tile: orders n0 .. n0 + cnt - 1 of vectors v0 .. v0 + nv - 1 of the batch into the ne accumulators
template <int VT>
void site_accumulate_vt(rsrec_t* h, const SitePlan& P, const SitePass& S, int PT) {
    const double2* ring = reinterpret_cast<const double2*>(P.ring);
    const double2 *coef = h->d_site_coef.as<double2>(), *w = h->d_site_w.as<double2>();
    const unsigned grid = (unsigned)((S.total + SITE_THREADS - 1) / SITE_THREADS);
    int* status = h->d_status.as<int>();
    auto go = [&](auto kern) { kern<<<grid, SITE_THREADS, 0, h->stream>>>(ring, coef, w, S, P.acc, status); };
    if (PT == 1) go(k_site_accum<VT, 1>);
    else if (PT == 2) go(k_site_accum<VT, 2>);
    else if constexpr (VT <= 4) {
        if (PT == 4) go(k_site_accum<VT, 4>);
        else if constexpr (VT <= 2) {
            if (PT == 8) go(k_site_accum<VT, 8>);
            else if constexpr (VT == 1) go(k_site_accum<1, 16>);
        }
    }
}
void site_accumulate(rsrec_t* h, const SitePlan& P, const SitePass& S) {
    if (P.VT == 1) site_accumulate_vt<1>(h, P, S, P.PT);
    else if (P.VT == 2) site_accumulate_vt<2>(h, P, S, P.PT);
    else if (P.VT == 4) site_accumulate_vt<4>(h, P, S, P.PT);
    else site_accumulate_vt<8>(h, P, S, P.PT);
}

// rsrec_chebyshev_site_map behind its argument checks.  Per batch of nb vectors: 2 lld + 1 launches (twice that with hoh) advance all of
// them through the ring; after every PT orders and after the last one, one pass per tile of VT vectors adds the ring's new orders into the
// accumulators.  Behind the last batch k_site_out writes the blocks, in place into device memory or slice by slice through the staging buffer.
int run_site_map(rsrec_t* h, const char* who, const SiteCall& A) {
    const int kk = h->kk, ne = A.ne, nmom = 2 * A.lld + 2;
    drop_resident(h);                                            // the call leaves no image, and what an earlier call left goes with the buffers
    h->kubo_diag_nvec = h->kubo_diag_ll = 0;
    release_kubo_buffers(h, false, true);
    // one host pass over the seeds: the conjugated coefficient every vector leaves on every atom (the last entry on an atom stays), cnorm,
    // and the divergence bound
    std::vector<double> table((size_t)2 * A.nvec * kk, 0.0), cn(kk, 0.0);
    {
        std::vector<int> s0; std::vector<double> cf;
        for (int v = 0; v < A.nvec; ++v) {
            whole_vector_seeds(A.S, v, s0, cf);
            double* tv = table.data() + (size_t)2 * v * kk;
            for (size_t k = 0; k < s0.size(); ++k) { tv[2 * s0[k]] = cf[2 * k]; tv[2 * s0[k] + 1] = -cf[2 * k + 1]; }
            for (int j = 0; j < kk; ++j) cn[j] += tv[2 * j] * tv[2 * j] + tv[2 * j + 1] * tv[2 * j + 1];
        }
    }
    double norm2 = 0.0;
    for (int j = 0; j < kk; ++j) norm2 += cn[j];
    const bool full_dev = A.d_full && is_device_ptr(A.d_full), diag_dev = A.d_diag && is_device_ptr(A.d_diag);
    const bool stage = (A.d_full && !full_dev) || (A.d_diag && !diag_dev);
    SitePlan P;
    XFER(site_plan(h, who, A, stage, P));
    XFER(site_reserve(h, who, P));
    HIPCK(h, h->d_status.reserve(64));
    HIPCK(h, hipMemsetAsync(h->d_status.p, 0, 64, h->stream));
    HIPCK(h, h->d_seed.reserve((size_t)A.S.nseed * 4));
    HIPCK(h, h->d_seedcoef.reserve((size_t)A.S.nseed * sizeof(double2)));
    HIPCK(h, h->d_site_coef.reserve((size_t)P.nbv * kk * sizeof(double2)));
    HIPCK(h, h->d_site_w.reserve((size_t)nmom * ne * sizeof(double2)));
    XFER(xfer_h2d(h, h->d_site_w.p, A.w, (size_t)nmom * ne * sizeof(double2)));
    WholeLatticeCall W;
    XFER(whole_lattice_begin(h, W, P.nbv, true));
    W.hps = P.hps;
    W.ev_begin = next_event(h);
    std::vector<std::pair<hipEvent_t, hipEvent_t>> acc_ev, out_ev;
    SitePass S{};
    S.slot_stride = P.slot / 2; S.vstride = P.velems / 2; S.total = (size_t)kk * BLK; S.dstride = P.dstride;
    S.nring = P.R; S.kk = kk; S.nmom = nmom; S.ne = ne; S.bound = 1000.0 * std::max(1.0, norm2);
    for (int iv0 = 0; iv0 < A.nvec; iv0 += P.nbv) {
        const int nb = std::min(P.nbv, A.nvec - iv0);
        double* r0 = P.ring_slot(0);
        HIPCK(h, hipMemsetAsync(r0, 0, P.slot * 8, h->stream));
        XFER(xfer_h2d(h, h->d_site_coef.p, table.data() + (size_t)2 * iv0 * kk, (size_t)nb * kk * sizeof(double2)));
        XFER(seed_whole_vectors<LayoutCI>(h, who, A.S, iv0, nb, r0, P.velems));
        whole_lattice_batch(W, nb, false);
        for (int n = 0, n0 = 0; n < nmom; ++n) {
            if (n >= 1) {
                const double* cur = P.ring_slot(n - 1);
                whole_lattice_apply_h(W, cur, P.ring_slot(n), cheb_epilogue(n == 1, cur, n >= 2 ? P.ring_slot(n - 2) : nullptr, A.a, A.b));
            }
            if (n - n0 + 1 == P.PT || n == nmom - 1) {
                hipEvent_t e0 = next_event(h);
                S.n0 = n0; S.slot0 = n0 % P.R; S.cnt = n - n0 + 1;
                for (int v0 = 0; v0 < nb; v0 += P.VT) {
                    S.v0 = v0; S.nv = std::min(P.VT, nb - v0);
                    site_accumulate(h, P, S);
                }
                acc_ev.emplace_back(e0, next_event(h));
                n0 = n + 1;
            }
        }
        HIPCK(h, hipGetLastError());
    }
    // the divergence word before anything is written: a diverged call returns the error and leaves the outputs alone
    const int rc_status = finish_status(h);
    if (rc_status) { (void)whole_lattice_end(h, W, true); return rc_status; }
    hipEvent_t o0 = next_event(h);
    const unsigned out_rows = (unsigned)std::min(kk, 4096);
    if (full_dev || diag_dev)
        k_site_out<LayoutCI><<<dim3(ne, out_rows), SITE_OUT_THREADS, 0, h->stream>>>(P.acc, P.dstride, 0, kk, ne, full_dev ? reinterpret_cast<double2*>(A.d_full) : nullptr,
                                                                                     diag_dev ? reinterpret_cast<double2*>(A.d_diag) : nullptr);
    if (stage)
        for (int j0 = 0; j0 < kk; j0 += SITE_STAGE_ATOMS) {
            const int nj = std::min(SITE_STAGE_ATOMS, kk - j0);
            double2* sf = A.d_full && !full_dev ? P.stage_full : nullptr;
            double2* sd = A.d_diag && !diag_dev ? P.stage_diag : nullptr;
            k_site_out<LayoutCI><<<dim3(ne, nj), SITE_OUT_THREADS, 0, h->stream>>>(P.acc, P.dstride, j0, nj, ne, sf, sd);
            if (sf) XFER(xfer_d2h(h, A.d_full + (size_t)j0 * ne * 2 * BLK, sf, (size_t)nj * ne * BLK * sizeof(double2)));
            if (sd) XFER(xfer_d2h(h, A.d_diag + (size_t)j0 * ne * 2 * NB, sd, (size_t)nj * ne * NB * sizeof(double2)));
        }
    HIPCK(h, hipGetLastError());
    out_ev.emplace_back(o0, next_event(h));
    if (A.cnorm) {
        if (is_device_ptr(A.cnorm)) HIPCK(h, hipMemcpyAsync(A.cnorm, cn.data(), (size_t)kk * sizeof(double), hipMemcpyHostToDevice, h->stream));
        else std::copy(cn.begin(), cn.end(), A.cnorm);
    }
    XFER(whole_lattice_end(h, W, true));
    for (auto& pr : acc_ev) h->t_site_ms[0] += ev_ms(pr.first, pr.second);
    for (auto& pr : out_ev) h->t_site_ms[1] += ev_ms(pr.first, pr.second);
    h->t_rest_ms = h->t_site_ms[0] + h->t_site_ms[1];
    return RSREC_OK;
}

}  // namespace

extern "C" int rsrec_chebyshev_site_map(rsrec_t* h, int nvec, int nseed, const int32_t* seed_atoms, const double* seed_coef, int lld, double a, double b, int ne,
                                        const double* w, double* d_full, double* d_diag, double* cnorm) {
    const char* who = "rsrec_chebyshev_site_map";
    int rc = check_ready(h, who);
    if (rc) return rc;
    if (nvec < 0 || lld < 1 || a == 0.0) return fail(h, RSREC_ERR_ARG, "%s: nvec < 0, lld < 1 or a == 0", who);
    if (nseed < 1 || nseed > h->kk) return fail(h, RSREC_ERR_ARG, "%s: nseed = %d outside 1..%d", who, nseed, h->kk);
    if (nvec > 0 && (!seed_atoms || !seed_coef)) return fail(h, RSREC_ERR_ARG, "%s: NULL seed_atoms or seed_coef", who);
    if (ne < 1 || ne > RSREC_SITE_MAP_NE_MAX) return fail(h, RSREC_ERR_ARG, "%s: ne = %d outside 1..%d", who, ne, RSREC_SITE_MAP_NE_MAX);
    if (!w) return fail(h, RSREC_ERR_ARG, "%s: NULL w", who);
    for (size_t q = 0; q < (size_t)2 * (2 * lld + 2) * ne; ++q)
        if (!std::isfinite(w[q])) return fail(h, RSREC_ERR_ARG, "%s: weight (%zu, %zu) is not finite", who, q / 2 % (2 * lld + 2) + 1, q / 2 / (2 * lld + 2) + 1);
    if (!d_full && !d_diag) return fail(h, RSREC_ERR_ARG, "%s: d_full and d_diag are both NULL", who);
    if (!h->s5_built) return fail(h, RSREC_ERR_ARG, "%s: lattice has too many neighbour slots for the SpMM kernel", who);
    XFER(check_seeds(h, who, seed_atoms, (size_t)nvec * nseed, 0));
    for (int c = 0; c < nvec; ++c)
        if (std::all_of(seed_atoms + (size_t)c * nseed, seed_atoms + (size_t)(c + 1) * nseed, [](int32_t s) { return s == 0; }))
            return fail(h, RSREC_ERR_ARG, "%s: vector %d has no seed", who, c + 1);
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    if (nvec == 0) return RSREC_OK;
    const SiteCall A{nvec, lld, ne, KuboSeeds{nseed, seed_atoms, seed_coef}, a, b, w, d_full, d_diag, cnorm};
    return run_site_map(h, who, A);
}

// ------------------------------------------------------------------------------------------------------------------
// Wave-packet propagation (kernels_evolve.hpp): psi(t) = U(t) r and chi(t) = [X, U(t)] r step by step, on the whole-lattice products of
// the Kubo calls; per record the projection of psi on the seed (kernels_lattice.hpp) and the Chebyshev moments of chi (kernels_shot.hpp's Grams)
namespace {

constexpr size_t EVO_EVENTS_MAX = 8192;      // pending timing events of a call before they are folded into the sums (run_evolve)
constexpr int EVO_ORDERS_DEFAULT = 16;       // what evolve_orders = 0 means: batched, the fastest of 1, 4, 16 in every measured configuration

struct EvoCall {
    int nvec;
    KuboSeeds S;
    double a, b;
    int korder;
    const double* w;
    int nt, stride, mom;
    double *ret, *m0_full, *m0_diag, *m_full, *m_diag;
};

// The device memory of a call, decided before anything is reserved (as shot_plan does).  Per vector in flight, with its p and its g chain:
// two state slots (psi | chi now, and the sums that become the next ones), the ring of R order slots, D p_n, and with hoh the chains' h psi
// and the two temporaries of the operator product.  The moment stage needs nothing of its own: the step ring is idle then and holds
// 2 R orders of the moment chains (they are nb chains wide, the step's slots 2 nb).
struct EvoPlan {
    bool fused = false;
    int P = 0, R = 0, Rm = 0, Pm = 0, nbv = 0;   // orders per accumulation pass, step-ring slots; moment-ring slots and orders per Gram flush; vectors in flight
    int ksteps_total = 0, ksplit = 0;
    size_t velems = 0, slot = 0, mslot = 0, pmax = 0;   // doubles of a vector, of a step slot (2 nbv chains), of a moment slot (nbv chains); projection partials per chain
    size_t bytes_work = 0, bytes_part = 0, bytes_out = 0;
    size_t off[6] = {0, 0, 0, 0, 0, 0};                  // complex elements: ret, m0_full, m0_diag, m_full, m_diag, end
    double *state[2] = {nullptr, nullptr}, *ring = nullptr, *dp = nullptr, *hps = nullptr, *p1 = nullptr, *p2 = nullptr;
    double2 *part = nullptr, *out = nullptr;
    double* step_slot(const double* x0, int n) const { return n == 0 ? const_cast<double*>(x0) : ring + (size_t)((n - 1) % R) * slot; }
    double* mom_slot(const double* l0, int n) const { return n == 0 ? const_cast<double*>(l0) : ring + (size_t)((n - 1) % Rm) * mslot; }
};

int evo_plan(rsrec_t* h, const char* who, const EvoCall& A, EvoPlan& P) {
    const int kk = h->kk;
    const bool hoh = h->hoh != 0;
    const long po = h->opt_evolve_orders <= 0 ? EVO_ORDERS_DEFAULT : std::min<long>(h->opt_evolve_orders, EVO_ORDERS_MAX);
    P.fused = po == 1; P.P = (int)po; P.R = P.fused ? 3 : P.P + 2;
    P.Rm = 2 * P.R; P.Pm = P.Rm - 2;
    P.velems = (size_t)(kk + 1) * BLD;
    P.ksteps_total = (int)((NB * (size_t)kk + 3) / 4);
    P.ksplit = shot_ksplit(P.ksteps_total);
    P.pmax = (size_t)kk / LATTICE_SPLIT_ATOMS + 2;
    P.bytes_part = (size_t)P.Pm * P.ksplit * BLK * 16;
    const size_t nv = (size_t)A.nvec, mo = (size_t)A.mom;
    const size_t n_out[5] = {(size_t)BLK * A.nt * nv, A.m0_full ? BLK * mo * nv : 0, A.m0_diag ? NB * mo * nv : 0, A.m_full ? BLK * mo * A.nt * nv : 0,
                             A.m_diag ? NB * mo * A.nt * nv : 0};
    for (int q = 0; q < 5; ++q) P.off[q + 1] = P.off[q] + n_out[q];
    P.bytes_out = P.off[5] * 16;
    size_t free_b = 0, total_b = 0;
    HIPCK(h, hipMemGetInfo(&free_b, &total_b));
    size_t reusable = h->d_lat_tab.bytes + h->d_lat_w.bytes + h->d_lat_part.bytes;
    for (int v = 0; v < 6; ++v) reusable += h->d_vec[v].bytes;
    for (auto& kb : h->d_kubo) reusable += kb.bytes;
    const double budget = 0.9 * (double)(free_b + reusable);
    auto vectors_for = [&](int nbv) { return (size_t)nbv * (4 + 2 * P.R + 1 + (hoh ? 4 : 0)); };
    auto need_for = [&](int nbv) {
        return (double)vectors_for(nbv) * P.velems * 8 + (double)nbv * ((double)P.pmax * BLK * 16 + (double)kk * 20 + 64) + (double)P.bytes_part + (double)P.bytes_out;
    };
    int nbv = (int)std::min<long>({(long)A.nvec, h->opt_kubo_vbatch > 0 ? h->opt_kubo_vbatch : KUBO_CHAINS_MAX, (long)(KUBO_CHAINS_MAX / 2)});
    while (nbv > 1 && need_for(nbv) > budget) --nbv;
    if (need_for(nbv) > budget)
        return fail(h, RSREC_ERR_DEVICE, "%s: %.0f bytes needed for one vector at a time on %d atoms (evolve_orders=%d, mom=%d, nt=%d), %.0f bytes free", who, need_for(1), kk,
                    P.P, A.mom, A.nt, (double)free_b);
    P.nbv = nbv; P.slot = (size_t)2 * nbv * P.velems; P.mslot = (size_t)nbv * P.velems; P.bytes_work = vectors_for(nbv) * P.velems * 8;
    return RSREC_OK;
}

// The plan's buffers out of the handle's Kubo buffers: d_kubo[0] the work vectors, [3] the Grams' slice partials, [4] the outputs of the whole
// call.  Everything is cleared: block kk of every vector stays the zero block, and nothing an earlier call left is ever read.
int evo_reserve(rsrec_t* h, const char* who, EvoPlan& P) {
    const size_t want[5] = {P.bytes_work, 0, 0, P.bytes_part, P.bytes_out};
    for (int v = 0; v < 6; ++v) h->d_vec[v].release();
    h->d_kubo[1].release(); h->d_kubo[2].release();
    XFER(reserve_kubo_buffers(h, want, who));
    double* at = h->d_kubo[0].as<double>();
    auto take = [&](size_t nv) { double* p = at; at += nv * P.velems; return p; };
    P.state[0] = take(2 * P.nbv); P.state[1] = take(2 * P.nbv);
    P.ring = take((size_t)2 * P.R * P.nbv);
    P.dp = take(P.nbv);
    if (h->hoh) { P.hps = take(2 * P.nbv); P.p1 = take(P.nbv); P.p2 = take(P.nbv); }
    P.part = h->d_kubo[3].as<double2>();
    P.out = h->d_kubo[4].as<double2>();
    HIPCK(h, hipMemsetAsync(h->d_kubo[0].p, 0, P.bytes_work, h->stream));
    HIPCK(h, hipMemsetAsync(h->d_kubo[4].p, 0, P.bytes_out, h->stream));
    return RSREC_OK;
}

// accumulation pass of the batched form (and of order 0 in the fused one): orders n0 .. n0 + cnt - 1 of the step into the sums y
void evo_accumulate(rsrec_t* h, const EvoPlan& P, int nb, const double* x0, int n0, int cnt, double* y) {
    const size_t total = (size_t)h->kk * BLK, vs = P.velems / 2;
    EvoOrders X;
    for (int p = 0; p < EVO_ORDERS_MAX; ++p) X.x[p] = reinterpret_cast<const double2*>(P.step_slot(x0, n0 + (p < cnt ? p : 0)));
    const double2* w = h->d_evo_w.as<double2>() + n0;
    auto go = [&](auto kern, int per_wg) {
        const dim3 grid((unsigned)((total + per_wg - 1) / per_wg), (unsigned)(2 * nb));
        kern<<<grid, EVO_THREADS, 0, h->stream>>>(X, cnt, vs, total, w, reinterpret_cast<double2*>(y));
    };
    if (cnt <= 1) go(k_evo_accum<1, 4>, EVO_THREADS * 4);
    else if (cnt <= 2) go(k_evo_accum<2, 4>, EVO_THREADS * 4);
    else if (cnt <= 4) go(k_evo_accum<4, 4>, EVO_THREADS * 4);
    else if (cnt <= 8) go(k_evo_accum<8, 2>, EVO_THREADS * 2);
    else go(k_evo_accum<16, 1>, EVO_THREADS);
}

// One step: the sums of the korder orders started from the state x0 = [psi | chi] into y (cleared here).  korder - 1 launches advance
// both chains of every vector, one operator product per order forms D p_n, and the per-order pass adds it into g(n + 1).
int evo_step(WholeLatticeCall& W, const EvoPlan& P, const EvoCall& A, int nb, const double* x0, double* y, std::vector<std::pair<hipEvent_t, hipEvent_t>>& pass_ev) {
    rsrec_t* h = W.h;
    const size_t total = (size_t)h->kk * BLK, vs = P.velems / 2;
    const double2* w = h->d_evo_w.as<double2>();
    const unsigned wgs = (unsigned)((total + EVO_THREADS * EVO_SOURCE_U - 1) / (EVO_THREADS * EVO_SOURCE_U));
    HIPCK(h, hipMemsetAsync(y, 0, P.slot * 8, h->stream));
    for (int n = 0, n0 = 0; n < A.korder; ++n) {
        hipEvent_t e0 = nullptr;
        if (n >= 1) {
            const double* cur = P.step_slot(x0, n - 1);
            double* nxt = P.step_slot(x0, n);
            whole_lattice_batch(W, 2 * nb, false);
            whole_lattice_apply_h(W, cur, nxt, cheb_epilogue(n == 1, cur, n >= 2 ? P.step_slot(x0, n - 2) : nullptr, A.a, A.b));
            whole_lattice_batch(W, nb, false);
            whole_lattice_apply_v(W, h->kubo_op_b[0], cur, P.dp);                        // D p_{n-1}: the p chains are the slot's first nb
            e0 = next_event(h);
            const double f = (n == 1 ? 1.0 : 2.0) / A.a;
            if (P.fused)
                k_evo_source<true><<<dim3(wgs, 2 * nb), EVO_THREADS, 0, h->stream>>>(reinterpret_cast<double2*>(nxt), reinterpret_cast<const double2*>(P.dp), f, vs, total, nb, 0,
                                                                                      w + n, reinterpret_cast<double2*>(y));
            else
                k_evo_source<false><<<dim3(wgs, nb), EVO_THREADS, 0, h->stream>>>(reinterpret_cast<double2*>(nxt), reinterpret_cast<const double2*>(P.dp), f, vs, total, nb, nb,
                                                                                   w + n, reinterpret_cast<double2*>(y));
        } else e0 = next_event(h);
        if (P.fused) { if (n == 0) evo_accumulate(h, P, nb, x0, 0, 1, y); }
        else if (n - n0 + 1 == P.P || n == A.korder - 1) { evo_accumulate(h, P, nb, x0, n0, n - n0 + 1, y); n0 = n + 1; }
        pass_ev.emplace_back(e0, next_event(h));
    }
    return RSREC_OK;
}

// The moment stage of nb chains that start at l0 (chi of the batch's vectors, or r for m0): m(:, :, n, iv, j0 + c) = L^H T_{n-1}(H~) L for
// n = 1 .. mom by a plain three-term chain, mom - 1 launches for all nb chains together; the orders collect in the idle step ring and every
// Pm of them one Gram launch per vector (two where the ring wraps) forms their blocks.  full / diag: (.., mom, nrec, nvec) images, either may be null.
void evo_moments(WholeLatticeCall& W, const EvoPlan& P, const EvoCall& A, int nb, const double* l0, int iv, int nrec, int j0, double2* full, double2* diag) {
    rsrec_t* h = W.h;
    const bool mfma = h->opt_kernels != 1;
    auto grams = [&](const double* w0, size_t ws, int q, int cnt) {          // orders q .. q + cnt - 1 lie at w0 + e ws
        for (int c = 0; c < nb; ++c) {
            const double* L = l0 + (size_t)c * P.velems;
            const double* Wc = w0 + (size_t)c * P.velems;
            const dim3 grid((unsigned)P.ksplit, (unsigned)cnt);
            if (mfma) k_shot_gram<<<grid, 64, 0, h->stream>>>(L, 0, Wc, ws, P.ksteps_total, P.ksplit, P.part);
            else k_shot_gram_valu<<<grid, SHOT_GRAM_VALU_THREADS, 0, h->stream>>>(L, 0, Wc, ws, P.ksteps_total, P.ksplit, P.part);
            k_shot_gram_reduce<<<cnt, SHOT_GRAM_VALU_THREADS, 0, h->stream>>>(P.part, P.ksplit, A.mom, iv, nrec, j0 + c, full ? full + (size_t)q * BLK : nullptr,
                                                                             diag ? diag + (size_t)q * NB : nullptr);
        }
    };
    whole_lattice_batch(W, nb, false);
    grams(l0, 0, 0, 1);
    for (int n = 1, n0 = 1; n < A.mom; ++n) {
        const double* cur = P.mom_slot(l0, n - 1);
        whole_lattice_apply_h(W, cur, P.mom_slot(l0, n), cheb_epilogue(n == 1, cur, n >= 2 ? P.mom_slot(l0, n - 2) : nullptr, A.a, A.b));
        if (n - n0 + 1 < P.Pm && n != A.mom - 1) continue;
        for (int q = n0; q <= n;) {
            const int s = (q - 1) % P.Rm, cnt = std::min(n - q + 1, P.Rm - s);
            grams(P.ring + (size_t)s * P.mslot, P.mslot, q, cnt);
            q += cnt;
        }
        n0 = n + 1;
    }
}

// rsrec_chebyshev_evolve behind its argument checks.  Per batch of nb vectors: chains 0 .. nb - 1 carry psi, chains nb .. 2 nb - 1 chi; the
// two state slots swap roles after every step.  SpMM launches of a batch: nt stride (korder - 1) (1 + 1) for the steps, (1 + nrec) (mom - 1)
// for the moment stages (nrec = nt if m_* is asked for, the 1 if m0_* is); with hoh every H product is two launches and every D product three.
int run_evolve(rsrec_t* h, const char* who, const EvoCall& A) {
    const int kk = h->kk, nvec = A.nvec;
    h->kubo_diag_nvec = h->kubo_diag_ll = 0;                       // (d_kubo[4] is about to be overwritten)
    release_kubo_buffers(h, false, true);
    EvoPlan P;
    XFER(evo_plan(h, who, A, P));
    XFER(evo_reserve(h, who, P));
    HIPCK(h, h->d_seed.reserve((size_t)A.S.nseed * 4));
    HIPCK(h, h->d_seedcoef.reserve((size_t)A.S.nseed * sizeof(double2)));
    HIPCK(h, h->d_evo_w.reserve((size_t)A.korder * sizeof(double2)));
    XFER(xfer_h2d(h, h->d_evo_w.p, A.w, (size_t)A.korder * sizeof(double2)));
    const size_t n_list = (size_t)P.nbv * kk, n_off = (size_t)P.nbv * 2;
    HIPCK(h, h->d_lat_tab.reserve((n_list + 2 * n_off) * sizeof(int)));
    HIPCK(h, h->d_lat_w.reserve(n_list * sizeof(double2)));
    HIPCK(h, h->d_lat_part.reserve((size_t)P.nbv * P.pmax * BLK * sizeof(double2)));
    int *d_list = h->d_lat_tab.as<int>(), *d_seg = d_list + n_list, *d_split = d_seg + n_off;
    double2* d_w = h->d_lat_w.as<double2>();
    double2* partial = h->d_lat_part.as<double2>();
    double2 *ret = P.out + P.off[0], *m0f = A.m0_full ? P.out + P.off[1] : nullptr, *m0d = A.m0_diag ? P.out + P.off[2] : nullptr;
    double2 *mf = A.m_full ? P.out + P.off[3] : nullptr, *md = A.m_diag ? P.out + P.off[4] : nullptr;
    WholeLatticeCall W;
    XFER(whole_lattice_begin(h, W, 2 * P.nbv, true));
    W.hps = P.hps; W.p1 = P.p1; W.p2 = P.p2;
    W.ev_begin = next_event(h);
    const LatticeCall LC{nvec, 0, 1, A.S, nullptr, A.a, A.b, nullptr};
    LatticeBatchLists T;
    std::vector<double> bound(nvec, 0.0);
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pass_ev, rec_ev;
    // The events of a long run are folded into the sums and given back to the pool whenever more than EVO_EVENTS_MAX are pending (checked
    // behind every step and every record, never inside a timed span): a call of thousands of steps holds a bounded number of events --
    // about EVO_EVENTS_MAX plus those of one step or one moment stage -- at the price of one stream synchronisation per fold.
    const size_t ev_base = h->ev_used;
    double hop_ms = 0.0, hop_launches = 0.0;
    auto fold_events = [&](bool force) {
        if (!force && h->ev_used - ev_base <= EVO_EVENTS_MAX) return (int)RSREC_OK;
        HIPCK(h, hipStreamSynchronize(h->stream));
        for (auto& pr : W.hop_ev) hop_ms += ev_ms(pr.first, pr.second);
        for (auto& pr : pass_ev) h->t_evo_ms[0] += ev_ms(pr.first, pr.second);
        for (auto& pr : rec_ev) h->t_evo_ms[1] += ev_ms(pr.first, pr.second);
        hop_launches += (double)W.hop_ev.size();
        W.hop_ev.clear(); pass_ev.clear(); rec_ev.clear();
        h->ev_used = ev_base;
        return (int)RSREC_OK;
    };
    auto run_batches = [&]() {
    for (int iv0 = 0; iv0 < nvec; iv0 += P.nbv) {
        const int nb = std::min(P.nbv, nvec - iv0);
        lattice_lists(h, LC, iv0, nb, T);
        if ((size_t)T.pstride > P.pmax) return fail(h, RSREC_ERR_DEVICE, "%s: split partials outside the planned buffer", who);
        std::copy(T.bound.begin(), T.bound.end(), bound.begin() + iv0);
        XFER(xfer_h2d(h, d_list, T.list.data(), (size_t)nb * kk * sizeof(int)));
        XFER(xfer_h2d(h, d_seg, T.seg_off.data(), (size_t)nb * 2 * sizeof(int)));
        XFER(xfer_h2d(h, d_split, T.split_off.data(), (size_t)nb * 2 * sizeof(int)));
        XFER(xfer_h2d(h, d_w, T.weight.data(), (size_t)nb * kk * sizeof(double2)));
        const LatticeLists LL{d_list, d_w, d_seg, d_split, kk, 1, T.pstride};
        int cur = 0;
        HIPCK(h, hipMemsetAsync(P.state[0], 0, P.slot * 8, h->stream));                  // psi(0) = r into the p chains, chi(0) = 0
        XFER(seed_whole_vectors<LayoutCI>(h, who, A.S, iv0, nb, P.state[0], P.velems));
        if (m0f || m0d) {
            hipEvent_t e0 = next_event(h);
            evo_moments(W, P, A, nb, P.state[0], 0, 1, iv0, m0f, m0d);
            rec_ev.emplace_back(e0, next_event(h));
        }
        for (int s = 0; s < A.nt; ++s) {
            for (int k = 0; k < A.stride; ++k) {
                XFER(evo_step(W, P, A, nb, P.state[cur], P.state[1 - cur], pass_ev));
                cur = 1 - cur;
                XFER(fold_events(false));
            }
            HIPCK(h, hipGetLastError());
            hipEvent_t e0 = next_event(h);
            k_lattice_project<<<dim3(T.pstride, nb), LATTICE_THREADS, 0, h->stream>>>(LL, P.state[cur], P.velems, partial);
            k_lattice_reduce<LayoutCI><<<dim3(1, nb, LATTICE_RWG), 64, 0, h->stream>>>(LL, partial, iv0, s, A.nt, ret);
            if (mf || md) evo_moments(W, P, A, nb, P.state[cur] + (size_t)nb * P.velems, s, A.nt, iv0, mf, md);
            rec_ev.emplace_back(e0, next_event(h));
            XFER(fold_events(false));
        }
        HIPCK(h, hipGetLastError());
    }
    return (int)RSREC_OK;
    };
    // a failure in the middle of the batches leaves with nothing queued on the stream
    if (const int rc_run = run_batches()) { (void)hipStreamSynchronize(h->stream); (void)hipGetLastError(); return rc_run; }
    // the divergence test on ret before anything is written: a diverged call returns the error and leaves the outputs alone
    std::vector<double> hret(2 * (P.off[1] - P.off[0]));
    XFER(xfer_d2h(h, hret.data(), ret, hret.size() * 8));
    XFER(fold_events(true));
    XFER(whole_lattice_end(h, W, true));                           // (every launch span is folded: total_ms from the call's first event)
    h->t_hop_ms = hop_ms; h->n_hop_launch = hop_launches;
    h->t_rest_ms = h->t_evo_ms[0] + h->t_evo_ms[1];
    const size_t per_vec = (size_t)BLK * A.nt;
    for (int v = 0; v < nvec; ++v)
        for (size_t q = 0; q < per_vec; ++q) {
            const double re = hret[2 * (v * per_vec + q)], im = hret[2 * (v * per_vec + q) + 1];
            if (!(std::hypot(re, im) <= bound[v]))
                return fail(h, RSREC_ERR_DIVERGED, "%s: the projection of vector %d on its seed left 1000 max(1, sum |c|^2) at record %zu. Check the weights and a, b", who, v + 1,
                            q / BLK + 1);
        }
    auto deliver = [&](double* dst, const double2* src, size_t n) {
        if (!dst) return (int)RSREC_OK;
        if (is_device_ptr(dst)) { HIPCK(h, hipMemcpyAsync(dst, src, n * 16, hipMemcpyDeviceToDevice, h->stream)); return (int)RSREC_OK; }
        return xfer_d2h(h, dst, src, n * 16);
    };
    if (A.ret && !is_device_ptr(A.ret)) std::copy(hret.begin(), hret.end(), A.ret);
    else XFER(deliver(A.ret, ret, P.off[1] - P.off[0]));
    XFER(deliver(A.m0_full, m0f, P.off[2] - P.off[1]));
    XFER(deliver(A.m0_diag, m0d, P.off[3] - P.off[2]));
    XFER(deliver(A.m_full, mf, P.off[4] - P.off[3]));
    XFER(deliver(A.m_diag, md, P.off[5] - P.off[4]));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return RSREC_OK;
}

}  // namespace

extern "C" int rsrec_chebyshev_evolve(rsrec_t* h, int nvec, int nseed, const int32_t* seed_atoms, const double* seed_coef, double a, double b, const double* d_op,
                                      const double* do_op, int korder, const double* w, int nt, int stride, int mom, double* ret, double* m0_full, double* m0_diag,
                                      double* m_full, double* m_diag) {
    if (!h) return RSREC_ERR_ARG;
    const char* fn = "rsrec_chebyshev_evolve";
    XFER(check_ready(h, fn));
    if (korder < 2 || korder > RSREC_EVOLVE_KORDER_MAX) return fail(h, RSREC_ERR_ARG, "%s: korder=%d is not in 2..%d", fn, korder, RSREC_EVOLVE_KORDER_MAX);
    if (nt < 1 || nt > RSREC_EVOLVE_NT_MAX) return fail(h, RSREC_ERR_ARG, "%s: nt=%d is not in 1..%d", fn, nt, RSREC_EVOLVE_NT_MAX);
    if (stride < 1 || stride > RSREC_EVOLVE_STRIDE_MAX) return fail(h, RSREC_ERR_ARG, "%s: stride=%d is not in 1..%d", fn, stride, RSREC_EVOLVE_STRIDE_MAX);
    if (mom < 0 || mom > RSREC_EVOLVE_MOM_MAX) return fail(h, RSREC_ERR_ARG, "%s: mom=%d is not in 0..%d", fn, mom, RSREC_EVOLVE_MOM_MAX);
    if (!w || !d_op) return fail(h, RSREC_ERR_ARG, "%s: w and d_op must be given", fn);
    if (!ret && !m0_full && !m0_diag && !m_full && !m_diag) return fail(h, RSREC_ERR_ARG, "%s: every output is NULL", fn);
    if (mom == 0 && (m0_full || m0_diag || m_full || m_diag)) return fail(h, RSREC_ERR_ARG, "%s: mom=0 forms ret only: the moment outputs must be NULL", fn);
    if (nvec < 0 || nseed < 1 || a == 0.0 || (nvec > 0 && (!seed_atoms || !seed_coef))) return fail(h, RSREC_ERR_ARG, "%s: bad argument", fn);
    if (h->hoh && !do_op) return fail(h, RSREC_ERR_ARG, "%s: hoh requires do_op", fn);
    if (!h->s5_built) return fail(h, RSREC_ERR_ARG, "%s: lattice has too many neighbour slots for the SpMM kernel", fn);
    for (size_t q = 0; q < 2 * (size_t)korder; ++q)
        if (!std::isfinite(w[q])) return fail(h, RSREC_ERR_ARG, "%s: weight %zu is not finite", fn, q / 2 + 1);
    XFER(check_seeds(h, fn, seed_atoms, (size_t)nvec * nseed, 0));
    for (int c = 0; c < nvec; ++c)
        if (std::all_of(seed_atoms + (size_t)c * nseed, seed_atoms + (size_t)(c + 1) * nseed, [](int32_t s) { return s == 0; }))
            return fail(h, RSREC_ERR_ARG, "%s: vector %d has no seed", fn, c + 1);
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    if (nvec == 0) return RSREC_OK;
    XFER(build_kubo_operator(h, h->kubo_op_b[0], d_op, do_op));
    if (h->hoh && h->nmax > 0) XFER(build_kubo_hbulk(h));
    const EvoCall A{nvec, KuboSeeds{nseed, seed_atoms, seed_coef}, a, b, korder, w, nt, stride, mom, ret, m0_full, m0_diag, m_full, m_diag};
    return run_evolve(h, fn, A);
}

extern "C" int rsrec_scalar_lanczos(rsrec_t* h, int nsites, const int32_t* seed_atoms, int lld, int llmax, double* a, double* b2) {
    int rc = check_ready(h, "rsrec_scalar_lanczos");
    if (rc) return rc;
    if (nsites < 0 || lld < 1 || llmax < lld || !a || !b2 || (nsites > 0 && !seed_atoms)) return fail(h, RSREC_ERR_ARG, "rsrec_scalar_lanczos: bad argument");
    XFER(check_seeds(h, "rsrec_scalar_lanczos", seed_atoms, (size_t)nsites, 1));
    HIPCK(h, hipSetDevice(h->device));
    reset_timing(h);
    std::fill(a, a + (size_t)llmax * NB * nsites, 0.0);
    std::fill(b2, b2 + (size_t)llmax * NB * nsites, 0.0);
    if (nsites == 0) return RSREC_OK;
    if (h->nsp != 1) {
        // hop() is a no-op unless nsp = 1 (recursion.f90:3326-3415): a stays 0 and crecal (:3466) divides by sqrt(0),
        // so the reference returns b2 = (1, 0, 0, NaN, NaN, ...).  Mirrored, not "fixed".
        for (size_t q = 0; q < (size_t)NB * nsites; ++q) {
            b2[q * llmax] = 1.0;
            for (int ll = 3; ll < lld; ++ll) b2[q * llmax + ll] = std::nan("");
        }
        return RSREC_OK;
    }
    const int kk = h->kk;
    const int nsteps = lld - 1;
    const int nlev = nsteps + 1;
    const size_t velems = (size_t)kk * NB;
    const int B = (int)std::min<long>(nsites, h->opt_batch > 0 ? h->opt_batch : 16);
    const int nblk = (int)std::min<long>(std::max<long>(1, (kk + TILE_ATOMS - 1) / TILE_ATOMS), 64);
    const int nch = B * NB;
    release_kubo_buffers(h, true, true);
    for (int v = 0; v < 2; ++v) HIPCK(h, h->d_vec[v].reserve((size_t)nch * velems * sizeof(double2)));
    HIPCK(h, h->d_scal.reserve((size_t)nch * (nblk + 2 * (size_t)lld) * sizeof(double) + 64));
    HIPCK(h, h->d_seed.reserve((size_t)nch * 2 * 4));
    double2* psi = h->d_vec[0].as<double2>();
    double2* pmn = h->d_vec[1].as<double2>();
    double* part = h->d_scal.as<double>();
    double* ca = part + (size_t)nch * nblk;
    double* cb = ca + (size_t)nch * lld;
    const DevProblem P = make_problem(h);
    hipEvent_t ev_begin = next_event(h);
    std::vector<double> ha((size_t)nch * lld), hb((size_t)nch * lld);
    for (int c0 = 0; c0 < nsites; c0 += B) {
        const int nb = std::min(B, nsites - c0);
        const int nc = nb * NB;
        std::vector<int> seeds0(nb), so((size_t)nc * 2);
        for (int q = 0; q < nb; ++q) {
            seeds0[q] = seed_atoms[c0 + q] - 1;
            for (int l = 0; l < NB; ++l) { so[2 * (q * NB + l)] = seeds0[q]; so[2 * (q * NB + l) + 1] = l; }
        }
        rc = upload_regions(h, seeds0.data(), nb, 1, nlev, nsteps, false, false);
        if (rc) return rc;
        h->n_atom_steps += h->cur_entry->atom_steps * NB;
        XFER(xfer_h2d(h, h->d_seed.p, so.data(), so.size() * 4));
        HIPCK(h, hipStreamSynchronize(h->stream));
        ChainView CV;
        chain_views(h, velems, NB, CV);
        for (int v = 0; v < 2; ++v) HIPCK(h, hipMemsetAsync(h->d_vec[v].p, 0, (size_t)nc * velems * sizeof(double2), h->stream));
        HIPCK(h, hipMemsetAsync(ca, 0, (size_t)nch * 2 * lld * sizeof(double), h->stream));
        k_scalar_seed<<<nc, 64, 0, h->stream>>>(psi, velems, h->d_seed.as<int>(), cb, lld);
        const dim3 grid(nblk, nc);
        for (int ll = 0; ll < nsteps; ++ll) {
            k_scalar_hop<<<grid, NTHREADS, 0, h->stream>>>(P, CV, ll + 1, psi, pmn, part);
            k_scalar_reduce<<<nc, 64, 0, h->stream>>>(part, nblk, ca, lld, ll);
            k_scalar_orth<<<grid, NTHREADS, 0, h->stream>>>(kk, CV, ll + 1, psi, pmn, ca, lld, ll, part);
            k_scalar_reduce<<<nc, 64, 0, h->stream>>>(part, nblk, cb, lld, ll + 1);
            k_scalar_update<<<grid, NTHREADS, 0, h->stream>>>(kk, CV, ll + 1, psi, pmn, cb, lld, ll);
            h->n_hop_launch += 1;
        }
        HIPCK(h, hipGetLastError());
        XFER(xfer_d2h(h, ha.data(), ca, (size_t)nc * lld * sizeof(double)));
        XFER(xfer_d2h(h, hb.data(), cb, (size_t)nc * lld * sizeof(double)));
        HIPCK(h, hipStreamSynchronize(h->stream));
        for (int q = 0; q < nc; ++q)
            for (int ll = 0; ll < lld; ++ll) {
                a[(size_t)llmax * ((size_t)c0 * NB + q) + ll] = ha[(size_t)q * lld + ll];
                b2[(size_t)llmax * ((size_t)c0 * NB + q) + ll] = hb[(size_t)q * lld + ll];
            }
    }
    hipEvent_t ev_end = next_event(h);
    HIPCK(h, hipStreamSynchronize(h->stream));
    h->t_total_ms = ev_ms(ev_begin, ev_end);
    return RSREC_OK;
}
