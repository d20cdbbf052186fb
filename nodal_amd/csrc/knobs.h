// Every environment variable the native library reads, declared once: the only file under csrc/ that calls getenv.
// Plain host C++17 (fastcsv.cpp and the host tools that include slu_analyse.h are built without HIP).
//
// One value type per parse rule; its now() reads the environment at that moment and applies the rule.  Whether a
// value is latched is the call site's business: `static const bool x = knob::X.now();` reads once per process, a
// plain `knob::X.now()` reads on every pass.  Clamps and value checks stay at the site too.
//
// One declaration per knob and per line: `inline constexpr <Kind> <NAME>{"<variable>"[, <default>]};  // <when>: <what>`
// (tests/test_knobs.py reads these lines and holds DESIGN.md's table of section 5 against them).  <when> is
//   process  latched on first use, for the life of the process
//   call     read on every call of the function named
//   create   read when a handle (nodal_create) or a hierarchy is created
//   load     read when the library is loaded
//   mixed    latched at some sites and read per call at others, as named
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <optional>

namespace knob {

struct Present {  // on if the variable is set to anything, "0" and "" included
    const char *name;
    bool now() const { return getenv(name) != nullptr; }
};
struct OnUnless0 {  // on, unless the variable is set and parses to 0 ("", "abc" parse to 0)
    const char *name;
    bool now() const { const char *e = getenv(name); return !(e && atoi(e) == 0); }
};
struct OffUnlessNon0 {  // off, unless the variable parses to something else than 0
    const char *name;
    bool now() const { const char *e = getenv(name); return e && atoi(e) != 0; }
};
struct OnIfSet0 {  // on only if the variable is set and parses to 0
    const char *name;
    bool now() const { const char *e = getenv(name); return e != nullptr && atoi(e) == 0; }
};
struct Level {  // 0 if unset; set to anything: at least 1
    const char *name;
    int now() const {
        const char *e = getenv(name);
        if (!e) return 0;
        const int v = atoi(e);
        return v > 1 ? v : 1;
    }
};
struct Int {
    const char *name;
    int dflt;
    int now() const { const char *e = getenv(name); return e ? atoi(e) : dflt; }
};
struct Int64 {
    const char *name;
    int64_t dflt;
    int64_t now() const { const char *e = getenv(name); return e ? atoll(e) : dflt; }
};
struct Double {
    const char *name;
    double dflt;
    double now() const { const char *e = getenv(name); return e ? atof(e) : dflt; }
};
// A number without a default of its own: empty if the variable is unset (the site keeps what it has, or names its
// own default with value_or).
struct IntIfSet {
    const char *name;
    std::optional<int> now() const { const char *e = getenv(name); return e ? std::optional<int>(atoi(e)) : std::nullopt; }
};
struct Int64IfSet {
    const char *name;
    std::optional<int64_t> now() const { const char *e = getenv(name); return e ? std::optional<int64_t>(atoll(e)) : std::nullopt; }
};
struct DoubleIfSet {
    const char *name;
    std::optional<double> now() const { const char *e = getenv(name); return e ? std::optional<double>(atof(e)) : std::nullopt; }
};
struct Text {  // the variable's text, parsed at the site; null if unset
    const char *name;
    const char *now() const { return getenv(name); }
};

// ---- every route
inline constexpr Present TRACE{"NODAL_TRACE"};  // mixed: progress and phase times on stderr; latched in sagg.hip, sparse.hip (sparse_solve, amg_fcg_solve_ex), presolve.hip (presolve_plan, presolve_build_reduced), dense_lu.hip; per call in the other files and in presolve_solve
inline constexpr Level POISON{"NODAL_POISON"};  // process: 1 growing buffers are filled with 0xFF instead of zeros, 2 every scratch buffer too at each solve entry
inline constexpr Present NOFILL{"NODAL_NOFILL"};  // process: growing buffers are not filled at all
inline constexpr Present NANCHECK{"NODAL_NANCHECK"};  // process: non-finite values are reported at named points of the general path
inline constexpr Double WAIT_TIMEOUT_S{"NODAL_WAIT_TIMEOUT_S", 60.0};  // process: bound of every host wait in seconds; 0 or less: the runtime's own blocking wait
inline constexpr Text STREAM_PRIORITY{"NODAL_STREAM_PRIORITY"};  // create: "normal" gives the main stream the default priority instead of the highest
inline constexpr IntIfSet EXTRA_STREAMS{"NODAL_EXTRA_STREAMS"};  // create: overrides the handle option of the same name (setup fork, direct-route lanes)
inline constexpr IntIfSet HOST_THREADS{"NODAL_HOST_THREADS"};  // call: host threads of the presolve's loops, the direct analysis and the CSV reader (at least 1; unset: the machine's)
inline constexpr IntIfSet CSV_CHUNKS{"NODAL_CSV_CHUNKS"};  // call: chunks the CSV reader cuts a file into (testing: more than a small file deserves)
// ---- 3.1 stamping
inline constexpr OnUnless0 FOLD_STREAM{"NODAL_FOLD_STREAM"};  // call: 0 folds the values by one lane per entry instead of the streaming fold
inline constexpr OffUnlessNon0 COUNT_LDS{"NODAL_COUNT_LDS"};  // process: 1 pre-aggregates a tile's rows in LDS while counting (slower; the cross-check)
// ---- 3.2 dense solve
inline constexpr IntIfSet DENSE_BLOCKINV{"NODAL_DENSE_BLOCKINV"};  // create: 0 sends passive dense systems through the no-pivot LU instead of the block elimination
inline constexpr IntIfSet GJ_SCALAR{"NODAL_GJ_SCALAR"};  // create: 1 scalar, 2 rank-4 MFMA instead of the rank-16 two-level Gauss-Jordan
inline constexpr OnUnless0 GJ_DPP{"NODAL_GJ_DPP"};  // process: 0 exchanges by ds_bpermute in the in-wave 16 x 16 inverse instead of v_readlane / DPP (the same bits)
inline constexpr OnUnless0 BI_SYM{"NODAL_BI_SYM"};  // process: 0 full instead of symmetric block elimination
inline constexpr OnIfSet0 BI_MASKED{"NODAL_BI_MASKED"};  // process: 0 runs the bulk updates on all CUs instead of the CU-masked stream
inline constexpr Int PANEL_CUS{"NODAL_PANEL_CUS", 32};  // create: CUs the masked bulk stream leaves to the chain, clamped to 0..224 (read when a handle's side streams are made)
inline constexpr Int64 BI_UNMASK_ROWS{"NODAL_BI_UNMASK_ROWS", 0};  // process: rows left above which the bulk update takes all CUs (experiment, off)
inline constexpr OnUnless0 BI_EARLY_COPY{"NODAL_BI_EARLY_COPY"};  // process: 0 no early copy of the next block's columns in the symmetric chain
inline constexpr Int BI_FIRST_BLOCKS{"NODAL_BI_FIRST_BLOCKS", 2};  // process: diagonal blocks ahead whose columns of W are updated first
inline constexpr Text BI_SWITCH{"NODAL_BI_SWITCH"};  // call: rows left at which the block width drops to 256 (4608)
inline constexpr Text BI_SWITCH2{"NODAL_BI_SWITCH2"};  // call: rows left at which the block width drops to 128 (0: never)
inline constexpr Text BI_WIDTH{"NODAL_BI_WIDTH"};  // call: 128, 512 or (anything else) 256 as the one block width
inline constexpr IntIfSet GEPP_PANEL{"NODAL_GEPP_PANEL"};  // create: 0 partial pivoting by two launches per column instead of the panel kernel
inline constexpr Int GEPP_MAX{"NODAL_GEPP_MAX", 1280};  // load: largest system for LAPACK-ordered partial pivoting (above: tournament)
inline constexpr Present GEPP_PROBE{"NODAL_GEPP_PROBE"};  // process: clock stamps of the panel kernel's phases
// ---- 3.3 sparse SPD path
inline constexpr Int64IfSet FCG_MAXIT{"NODAL_FCG_MAXIT"};  // call: iteration limit; the sites' own defaults: 5000 (sparse.hip), 2000 (sagg.hip), four times the last solve and at least 64 (sagg_multi.h)
inline constexpr OnUnless0 FCG_HOST_SUM{"NODAL_FCG_HOST_SUM"};  // call: 0 takes convergence from the device's flag only (one cycle later)
inline constexpr Double FCG_LOOK{"NODAL_FCG_LOOK", 0.75};  // process: share of the predicted remaining iterations enqueued before the next look
inline constexpr OnUnless0 LOWDEG{"NODAL_LOWDEG"};  // call: 0 no elimination of low-degree nodes
inline constexpr IntIfSet LOWDEG_SHARE{"NODAL_LOWDEG_SHARE"};  // call: a round must remove n / k nodes (positive, else the caller's share)
inline constexpr Int64 LOWDEG_MIN{"NODAL_LOWDEG_MIN", 32};  // process: unknowns below which the elimination rounds stop
inline constexpr Present SPARSE_FORCE_DIRECT{"NODAL_SPARSE_FORCE_DIRECT"};  // call: every automatic sparse solve takes the direct route
inline constexpr Present SPARSE_CHILD_DIRECT{"NODAL_SPARSE_CHILD_DIRECT"};  // call: the reduced contexts' automatic sparse solves take the direct route
// ---- 3.3a smoothed aggregation
inline constexpr OnUnless0 SAGG{"NODAL_SAGG"};  // process: 0 plain-aggregation hierarchy only
inline constexpr OnUnless0 SA_REUSE{"NODAL_SA_REUSE"};  // process: 0 no values-only refresh (full setup every time)
inline constexpr OnUnless0 SA_FORK{"NODAL_SA_FORK"};  // mixed: 0 keeps the setup on one stream; latched in build_level, per call in the values-only refresh
inline constexpr Double SA_SPREAD{"NODAL_SA_SPREAD", 16.0};  // process: link spread above which a node counts as graded
inline constexpr Double SA_SHARE{"NODAL_SA_SHARE", 0.9};  // process: share of the diagonal above which one link counts as dominant
inline constexpr IntIfSet SA_MIS{"NODAL_SA_MIS"};  // process: independent-set rounds, clamped to 1..6 (unset: 6)
inline constexpr Text SA_OMEGA_P{"NODAL_SA_OMEGA_P"};  // process: "w0" or "w0,w1" prolongator weights of level 0 and of the coarse levels (0.70, 0.85)
inline constexpr Double SA_PADSLACK{"NODAL_SA_PADSLACK", 1.3};  // process: padding a fixed-width level may cost
inline constexpr OnUnless0 SA_D16{"NODAL_SA_D16"};  // process: 0 32-bit instead of 16-bit column deltas at level 0
inline constexpr Int SA_GG{"NODAL_SA_GG", 40};  // process: R entries per Galerkin group at level 0
inline constexpr Int64 SA_GCAP{"NODAL_SA_GCAP", 16384};  // process: most workgroups of the Galerkin product (each walks several rows)
inline constexpr Int SA_GROWS{"NODAL_SA_GROWS", 4};  // process: coarse rows per wavefront of the Galerkin sums at 16-slot levels: 0 one coarse row per wavefront, else four small ones
inline constexpr OnUnless0 SA_GDYN{"NODAL_SA_GDYN"};  // process: 0 the Galerkin groups of 64-slot levels are 16 R entries each instead of what fits the list
inline constexpr Int SA_GLIST{"NODAL_SA_GLIST", 1024};  // process: slots of the Galerkin product list at 64-slot levels under NODAL_SA_GDYN, clamped to 64..1024
inline constexpr Int SA_GSEG{"NODAL_SA_GSEG", 4};  // process: 1, 2 or 4 lane segments of the Galerkin accumulation
inline constexpr Text SA_NU{"NODAL_SA_NU"};  // call: e.g. "212" Jacobi sweeps per side at level 0 / 1 / deeper (1-3 each)
inline constexpr Int SA_KCYCLE{"NODAL_SA_KCYCLE", 1};  // process: 0 K-cycle off
inline constexpr Int SA_KLEVELS{"NODAL_SA_KLEVELS", 1};  // call: the K-cycle at the first k coarse levels
inline constexpr OnUnless0 SA_KFREEZE{"NODAL_SA_KFREEZE"};  // process: 0 the K-cycle's coefficients adaptive in every iteration
inline constexpr OnUnless0 SA_FUSE_DIR{"NODAL_SA_FUSE_DIR"};  // process: 0 direction update and outer SpMV as two launches
inline constexpr OffUnlessNon0 SA_GRAPH{"NODAL_SA_GRAPH"};  // process: 1 hipGraph replay of iteration pairs on a kept hierarchy
inline constexpr Text SA_FOLD_POST{"NODAL_SA_FOLD_POST"};  // process: levels that fold their first post-smoothing sweep into the prolongation: unset or "" levels of at most 524288 rows, "0" none, "1" all outside the tail, "l0,l2" those named
inline constexpr OffUnlessNon0 SA_FOLD_CHECK{"NODAL_SA_FOLD_CHECK"};  // process: 1 with NODAL_TRACE: the setup prints the scaled difference of the folded launch and the two it replaces
inline constexpr OnUnless0 SA_FOLD_VISIT{"NODAL_SA_FOLD_VISIT"};  // process: 0 the level directly above the dense tail keeps its six launches per visit instead of three
inline constexpr Int64 SA_VISIT_CAP{"NODAL_SA_VISIT_CAP", 16777216};  // process: bytes of the dense P2^T above which that level keeps its six launches
inline constexpr OffUnlessNon0 SA_VISIT_CHECK{"NODAL_SA_VISIT_CHECK"};  // process: 1 with NODAL_TRACE: the setup prints the scaled difference of the three-launch visit and the six launches it replaces
inline constexpr OnUnless0 SA_RESTRICT_B{"NODAL_SA_RESTRICT_B"};  // process: 0 a level with one sweep per side keeps its residual and restriction launches instead of forming rc = W^T b beside the residual in one
inline constexpr OffUnlessNon0 SA_RESTRICT_CHECK{"NODAL_SA_RESTRICT_CHECK"};  // process: 1 with NODAL_TRACE: the setup prints the scaled difference of rc formed from b and by the two launches it replaces
inline constexpr OnUnless0 SA_TAIL_DENSE{"NODAL_SA_TAIL_DENSE"};  // process: 0 the tail walked by k_tail on every visit instead of applied as a dense operator
inline constexpr OffUnlessNon0 SA_TAIL_CHECK{"NODAL_SA_TAIL_CHECK"};  // process: 1 with NODAL_TRACE: the setup prints the scaled difference of both forms of the tail
inline constexpr Int SA_TAIL_NU{"NODAL_SA_TAIL_NU", 3};  // create: sweeps inside the LDS tail (at least 1)
inline constexpr Present TAIL_PROBE{"NODAL_TAIL_PROBE"};  // create: clock stamps of the tail kernel's phases (the k_tail path)
// ---- 3.3b plain aggregation
inline constexpr IntIfSet AMG_PASSES0{"NODAL_AMG_PASSES0"};  // create: coarsening passes at level 0
inline constexpr IntIfSet AMG_PASSES1{"NODAL_AMG_PASSES1"};  // create: coarsening passes at the coarse levels
inline constexpr IntIfSet AMG_SWEEPS0{"NODAL_AMG_SWEEPS0"};  // create: smoothing sweeps at level 0
inline constexpr IntIfSet AMG_BLOCK{"NODAL_AMG_BLOCK"};  // create: 0 point, 1 aggregate-block smoother (unset: by the count of graded links)
inline constexpr DoubleIfSet AMG_THETA{"NODAL_AMG_THETA"};  // create: strength bar below which a link may be cut (unset: 0.1 with the block smoother, else 0)
inline constexpr Present AMG_KEEP_DENSE{"NODAL_AMG_KEEP_DENSE"};  // create: keeps a first coarse level whose rows came out 4 x denser than the fine ones
inline constexpr Present AMG_NOTAIL{"NODAL_AMG_NOTAIL"};  // create: no LDS tail
inline constexpr IntIfSet AMG_KMAX{"NODAL_AMG_KMAX"};  // create: coarse level down to which the K-cycle runs (unset: by the levels' sizes)
// ---- 3.3c block sweeps and source sweeps
inline constexpr OnUnless0 PAIRS_BLOCK{"NODAL_PAIRS_BLOCK"};  // call: 0 pair sweeps one solve per pair
inline constexpr OnUnless0 PAIRS_FUNCTIONAL{"NODAL_PAIRS_FUNCTIONAL"};  // call: 0 the block sweep stops on the residual rule
inline constexpr Int PAIRS_DIRECT{"NODAL_PAIRS_DIRECT", -1};  // call: 1 pair sweeps through the sparse LU, 0 never, -1 by the number of pairs
inline constexpr Int64 PAIRS_DIRECT_MIN{"NODAL_PAIRS_DIRECT_MIN", 256};  // call: pairs from which a sweep takes the factor-once route
inline constexpr Double MULTI_BAR{"NODAL_MULTI_BAR", 1e-14};  // call: backward-error bar of the sparse-LU route of the multi-right-hand-side driver; negative: every column redone alone
inline constexpr OnUnless0 TNL_REUSE{"NODAL_TNL_REUSE"};  // call: 0 nodal_transient_nl assembles G in every Newton iteration, also where no diode's 1 / g moved (the same bits)
// ---- 3.4 general sparse path
inline constexpr IntIfSet PRESOLVE{"NODAL_PRESOLVE"};  // create: 0 branch equations stay in the system (full-system FGMRES / pivoted LU)
inline constexpr OnUnless0 PRESOLVE_KEEP{"NODAL_PRESOLVE_KEEP"};  // process: 0 one source the presolve cannot substitute ends it
inline constexpr IntIfSet FGMRES_WINDOW{"NODAL_FGMRES_WINDOW"};  // process: restart window of the full-system FGMRES (at least 2; unset: chosen by size)
// ---- 3.5 sparse direct route
inline constexpr Text DIRECT_NB{"NODAL_DIRECT_NB"};  // call: 16, 32, 48 or 64 columns per panel of the wide fronts (16)
inline constexpr Int DIRECT_LANES{"NODAL_DIRECT_LANES", 4};  // call: wide fronts factored side by side, clamped to 1..6
inline constexpr DoubleIfSet DIRECT_MAX_GB{"NODAL_DIRECT_MAX_GB"};  // call: memory the fronts may take (unset: half of what is free)
inline constexpr IntIfSet DIRECT_BIG_DIM{"NODAL_DIRECT_BIG_DIM"};  // process: front width above which a front is stepped with its level's wide ones (unset: 84)
inline constexpr OnUnless0 DIRECT_FRONT_LDS{"NODAL_DIRECT_FRONT_LDS"};  // call: 0 small fronts in global memory
inline constexpr Int DIRECT_LDS_BS{"NODAL_DIRECT_LDS_BS", 64};  // process: threads per front of the in-LDS kernel
inline constexpr OnUnless0 DIRECT_PANEL_REGS{"NODAL_DIRECT_PANEL_REGS"};  // call: 0 the streaming panel kernel
inline constexpr OnUnless0 DIRECT_BATCHED{"NODAL_DIRECT_BATCHED"};  // call: 0 per-front panel chains
inline constexpr OnUnless0 DIRECT_WAVE{"NODAL_DIRECT_WAVE"};  // call: 0 leaves by workgroups instead of wavefronts
inline constexpr Present DIRECT_LEVELS{"NODAL_DIRECT_LEVELS"};  // call: an event behind every level and a table of times, flops and bytes per level on stderr
inline constexpr OnUnless0 DIRECT_SUPER{"NODAL_DIRECT_SUPER"};  // process: 0 block steps instead of super steps in the triangular solves
inline constexpr OnUnless0 DIRECT_APPLY_STEPPED{"NODAL_DIRECT_APPLY_STEPPED"};  // process: 0 one workgroup per wide front in the triangular solves
inline constexpr OnUnless0 DIRECT_PEEL{"NODAL_DIRECT_PEEL"};  // process: 0 no leaves-first ordering
inline constexpr Int ND_DEPTH{"NODAL_ND_DEPTH", 4};  // process: levels of the threaded nested dissection
inline constexpr Int64 ND_PAR{"NODAL_ND_PAR", 20000};  // process: piece size from which the dissection's halves run on threads
inline constexpr Present SLU_DEBUG{"SLU_DEBUG"};  // call: the matching's augmenting paths on stderr

}  // namespace knob
