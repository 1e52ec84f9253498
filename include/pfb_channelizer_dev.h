/* pfb_channelizer_dev.h -- measurement and kernel-study entry points of libpfb_channelizer.
 *
 * NOT part of the drop-in boundary: nothing here replaces a reference interface, and an integrator
 * binds pfb_channelizer.h and pfb_iq_packet.h only.  These are the hooks bench.py, tools/ and the tests use to put a
 * yardstick next to a kernel's rate (copy kernels with the channelizer's byte mix and no arithmetic), to select a
 * registered kernel plan other than the default one for A/B runs, and to prove a property of the ABI itself (no C++
 * exception crosses it).  Same shared library, same C ABI rules (plain pointers and sizes, status codes, never throws).
 */
#ifndef PFB_CHANNELIZER_DEV_H
#define PFB_CHANNELIZER_DEV_H

#include "pfb_channelizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Options of pfb_set_option (pfb_channelizer.h) for kernel studies; every combination a kernel accepts produces the
 * same bits as the handle's default plan (tests/test_gpu_parity.py walks them).  All are per handle. */
enum pfb_dev_option {
  PFB_OPT_GRID = 7,        /* schedule 13: resident workgroups to launch, each walking runs b, b + G, ... (0 = one per run) */
  PFB_OPT_TILE_WAVES = 8,  /* schedules 2 / 3 / 8: waves, 4 / 7: wave pairs per workgroup (1 ... 16)                       */
  PFB_OPT_EXPERIMENT = 9,  /* timing experiments, 0 in production.  bit 0: nontemporal row loads in the one-dword-per-lane */
                           /* kernels; bit 1: the history update always as a launch of its own behind the channelizer      */
                           /* kernel (by default that kernel carries it for calls of at least one history with a frame);   */
                           /* bits 8-15: extra dynamic LDS in KiB for schedule 3 (an occupancy throttle).  None changes a  */
                           /* result bit.                                                                                   */
  PFB_OPT_VARIANT = 10     /* n-th fused kernel registered for this shape (0 = the default plan; PFB_ERR_UNSUPPORTED past   */
                           /* the last).  Rebuilds the handle's per-lane tables for the new plan; the filter state stays.   */
};

/* Device stream copy, read 1 : write 2 (configuration 2's traffic: int16 I/Q in, complex64 out), timed with HIP events
 * over `iters` launches after a warm-up: bytes moved per second, the "measured peak" next to the nominal roofline.
 * Allocates bytes_in of input and 2 * bytes_in of output scratch on device_id (-1 = current) for the call.  The kernel
 * is the fastest 1:2 shape tools/membench2 found on MI355X (short-lived 4-wave workgroups, two 256-byte rows per wave,
 * one 16-byte store per lane), so no channelizer kernel with this byte mix should beat the figure. */
int pfb_measure_stream_copy(int device_id, uint64_t bytes_in, int iters, double* bytes_per_sec);

/* The same for either byte mix of the channelizer and a given wave lifetime: a copy kernel with no arithmetic that
 * reads bytes_in and writes write_ratio x bytes_in (2: int16 I/Q -> complex64 at D = M; 4: int8 I/Q, or int16 at
 * D = M/2), every wave owning rows_per_wave consecutive 256-byte rows (even, >= 2).  What the memory system gives a
 * byte mix depends on how short-lived the waves are (0.78 / 0.75 of the nominal 8 TB/s at 2 rows, 0.63 / 0.64 at 512):
 * the bound bench.py prints next to each shape's fraction (roofline.copy_kernel_frac_by_byte_mix). */
int pfb_measure_mix_copy(int device_id, uint64_t bytes_in, uint32_t write_ratio, uint32_t rows_per_wave, int iters,
                         double* bytes_per_sec);

/* STFT timing study (tools/stft_rate.py --variant loadstore): 1 = the handle's fused kernel with its loads and stores
 * only -- the tile's span into LDS and the tile's outputs written from there, no window, no FFT -- so its time is the
 * memory part of the kernel's; the output is not an STFT.  0 = the real kernel again.  PFB_ERR_UNSUPPORTED for a handle
 * on the generic kernel.  Registered nowhere: pfb_stft_last_kernel names it pfb_stft_loadstore<...>. */
int pfb_stft_set_experiment(pfb_stft_handle* h, int experiment);

/* Which kernel folds the next calls of a pfb_fold handle: 0 = the library's choice (pfb_fold_plan.kernel), 1 =
 * fold_direct, 2 = fold_tile.  Both add every bin's cells in the definition's order and give the same bytes; the
 * tests run one handle through both, the meter (tools/fold_rate.py --tier) times both.  PFB_ERR_UNSUPPORTED for 2 when
 * bin_cells is not 8, 16, 32 or 64; PFB_ERR_BAD_ARG for any other value.  pfb_fold_last_kernel names what ran. */
int pfb_fold_set_tier(pfb_fold_handle* h, int tier);

/* Which kernels the next calls of a pfb_deint handle run.  histogram_tier: 0 = the library's choice
 * (pfb_deint_plan.histogram_kernel), 1 = the private LDS histogram (PFB_ERR_UNSUPPORTED when NB is above
 * pfb_deint_plan.lds_bins), 2 = global atomics.  marking_tier: 0 = the library's choice (the kept doubling
 * tables), 1 = the walk along b's chain in one lane, 2 = the tables.  All give the same bytes; the tests run one list
 * through them, the meter (tools/deint_rate.py) times them.  PFB_ERR_BAD_ARG for any other value.
 * pfb_deint_last_kernel names what ran. */
int pfb_deint_set_tier(pfb_deint_handle* h, int histogram_tier, int marking_tier);

/* Which kernel measures the pulses of the next calls of a pfb_mop handle: 0 = the library's choice by n
 * (pfb_mop_plan.group_min / split_min), 1 = mop_wave, 2 = mop_group, 3 = mop_split + mop_join, for every pulse
 * whatever its length.  grid_cap: the most workgroups of a launch, 0 = pfb_mop_plan.grid_cap again; stage_bytes: the
 * host route's staging chunk, 0 = pfb_mop_plan.stage_bytes again (a batch always takes one pulse at least).  For the
 * integer formats every tier gives the same bytes; the tests run one list through them, the meter (tools/mop_rate.py)
 * times them.  PFB_ERR_BAD_ARG for a tier outside 0 .. 3 or a grid_cap above 65536.  pfb_mop_last_kernel names what
 * ran. */
int pfb_mop_set_tier(pfb_mop_handle* h, int tier, uint32_t grid_cap, uint64_t stage_bytes);

/* Which kernel folds the next calls of a pfb_qfold handle, and how many cells one launch takes: tier 0 = the library's
 * choice (pfb_qfold_plan.kernel), 1 = qfold_direct, 2 = qfold_tile (PFB_ERR_UNSUPPORTED when bin_cells is not 8, 16, 32
 * or 64).  step_cells: cells per kernel launch and per staging step, 1 .. 2^24; 0 = 2^24 again.  A short step puts the
 * step boundary inside a short stream.  Both tiers and every step length give the same bytes.  PFB_ERR_BAD_ARG for any
 * other value.  pfb_qfold_last_kernel names what ran. */
int pfb_qfold_set_tier(pfb_qfold_handle* h, int tier, uint64_t step_cells);

/* Which kernel walks the windows in the next calls of a pfb_assoc handle: 0 = the library's choice
 * (pfb_assoc_plan.link_kernel), 1 = pfb_assoc_link_lds (PFB_ERR_UNSUPPORTED when window_items is above
 * pfb_assoc_plan.lds_window), 2 = pfb_assoc_link_global.  Both give the same bytes; the tests run one list through
 * them, the meter (tools/assoc_rate.py) times them.  PFB_ERR_BAD_ARG for any other value.  pfb_assoc_last_kernel names
 * what ran. */
int pfb_assoc_set_tier(pfb_assoc_handle* h, int tier);

/* Which kernel counts the cells in the next calls of a pfb_cluster handle: 0 = the library's choice
 * (pfb_cluster_plan.histogram_kernel), 1 = pfb_cluster_hist_lds (PFB_ERR_UNSUPPORTED when U V is above
 * pfb_cluster_plan.lds_cells), 2 = pfb_cluster_hist_global.  Both give the same bytes; the tests run one list through
 * them, the meter (tools/cluster_rate.py) times them.  PFB_ERR_BAD_ARG for any other value.  pfb_cluster_last_kernel
 * names what ran. */
int pfb_cluster_set_tier(pfb_cluster_handle* h, int tier);

/* The fused-kernel table, row by row in lookup order (host only, no device needed): what the tests walk, so that a
 * registered plan cannot go untested.  Rows of one (M, P, D, sample_format) are that shape's variants 0, 1, ... */
typedef struct {
  int M, P, D, sample_format;
  int variant;            /* index among the rows of this (M, P, D, format): what PFB_OPT_VARIANT takes */
  const char* name;       /* what pfb_last_kernel reports (static storage) */
  int default_schedule, magnitude_schedule, chunk_frames;
  int channel_major_ok;   /* 0: a channel-major handle on this plan goes by slabs + transpose */
  int default_frames_per_block; /* the tuned run length (before rounding to the chunk), what a long call runs with */
  int threads;            /* threads of the plan's FIR workgroup (run-length policy for short calls) */
} pfb_fast_plan_desc;
int pfb_fast_plan_count(void);
int pfb_fast_plan_info(int index, pfb_fast_plan_desc* out); /* PFB_ERR_BAD_ARG past the end or for NULL */

/* How the handle's last kernel launch went: what the launch policy actually handed to the kernel, so that a test can
 * tell which regime a call ran in without repeating the policy's arithmetic.  This is what was asked of the kernel;
 * which kernel ran, and on what grid, is pfb_last_entry below.  One call of pfb_process(_async) is one
 * launch (each staged chunk of a host-pointer call is one; pfb_process_shard_async makes two).  Host only, touches no
 * device; all zeros before the first launch.  A launch of the generic kernel reports fused = 0, its frames, and zeros. */
typedef struct {
  int fused;              /* 1: a fused plan (pfb_last_kernel names it), 0: the generic kernel or no launch yet */
  int schedule;           /* KernelParams.schedule as passed (-1: a fused channel-major launch, the kernel's own pick) */
  int frames_per_block;   /* run length passed to the kernel, after every per-call adjustment and rounding */
  int xcd_remap;          /* as passed: 0 off, 1 consecutive runs on one XCD, G > 1 in groups of G */
  int by_slabs;           /* 1: channel-major through frame-major slabs + the transpose kernel */
  int reserved;
  uint64_t frames;        /* frames of the launch */
  uint64_t runs;          /* ceil(frames / frames_per_block), summed over the slabs where it went by slabs */
  uint64_t slab_frames;   /* frames per slab (the last one may be shorter), 0 when not by slabs */
} pfb_launch_report;
int pfb_last_launch(const pfb_handle* h, pfb_launch_report* out); /* PFB_ERR_BAD_ARG for NULL */

/* The launch policy on its own (host only, no device needed): the report a handle on row plan_index of the table above
 * would store for a fused launch of `frames` frames with these options, layout, output type and compute-unit count --
 * the function launch_frames calls (pfb_launch_policy.h).  PFB_ERR_BAD_ARG for NULL, an index past the end or a
 * struct_size that is not sizeof(pfb_launch_request). */
typedef struct {
  uint32_t struct_size;
  int schedule;           /* PFB_OPT_SCHEDULE, -1 = default */
  int frames_per_block;   /* PFB_OPT_FRAMES_PER_BLOCK, 0 = default */
  int xcd_remap;          /* PFB_OPT_XCD_REMAP, -1 = per schedule */
  int channel_major;      /* the handle's layout */
  int magnitude;          /* PFB_FLAG_MAGNITUDE */
  int num_cus;            /* compute units of the device */
  int64_t slab_frames;    /* PFB_OPT_SLAB_FRAMES, 0 = default */
} pfb_launch_request;
int pfb_plan_launch(int plan_index, const pfb_launch_request* rq, uint64_t frames, pfb_launch_report* out);

/* The kernel entry: which kernel a launch resolved to.  pfb_launch_report is what was ASKED of the kernel -- the policy's
 * hand-down, "as passed" -- and a forced option the plan lacks falls through to another kernel without changing it; the
 * entry is what RAN.  Host only, touches no device.
 *
 * tag grammar (one place; static storage):   family [ "<" int { "," int } ">" ] { "+" role }
 *   family  sliding | tile | tile_t | shared | paired | pairs_sliding | overlap | teams | twin | seg (the fused kernels of
 *           pfb_fast_*.hpp), or generic
 *   ints    the kernel's integer template arguments behind the plan, as the source writes them: tile<waves>,
 *           tile_t<waves,chunks per wave>, shared<waves,run length>, paired<pairs,run length,min waves per SIMD>,
 *           pairs_sliding<pairs,min waves per SIMD>
 *   roles   what the instantiation has compiled in, in this order: cm = channel-major stores, ms = magnitudes staged in
 *           LDS, c64 / mag = complex or magnitude output, nt = nontemporal stores (after c64 only)
 *   e.g. paired<8,64,4>+c64, sliding+ms, tile_t<4,2>, seg+cm+mag.  Within one plan row two entries have the same tag if
 *   and only if they have the same kernel. */
typedef struct {
  int schedule;           /* of the kernel that ran (the list in pfb_fast.hpp): 0 when a forced schedule the plan lacks fell */
                          /* to its sliding runs, 8 / 2 / 0 where the report says -1; -1 = the generic kernel                */
  int threads;            /* per workgroup */
  uint32_t dyn_lds;       /* dynamic LDS in bytes */
  int reserved;
  uint64_t blocks;        /* workgroups launched (after PFB_OPT_GRID's cap) */
  uint64_t kernel;        /* address of the kernel's host stub: opaque, meaningful only for equality within a process */
  const char* tag;
} pfb_kernel_entry;
/* The entry of the handle's last kernel launch (by slabs: the last slab's frame-major launch; the transpose is not a
 * channelizer kernel).  All zeros and an empty tag before the first launch; PFB_ERR_BAD_ARG for NULL. */
int pfb_last_entry(const pfb_handle* h, pfb_kernel_entry* out);

/* The selection on its own, as pfb_plan_launch is the policy on its own (no device needed): runs the policy for
 * `launch` and `frames` on row plan_index, fills the kernel's parameters the way a handle with these options does and
 * returns the entry the row's select resolves them to.  By slabs it describes one full slab's launch.  A kernel of 0
 * means the plan has no kernel for the call (the launch would fail).  PFB_ERR_BAD_ARG for NULL, an index past the end
 * or a struct_size (either one) that does not match. */
typedef struct {
  uint32_t struct_size;
  int plan_index;
  pfb_launch_request launch; /* what the policy sees */
  int tile_waves;         /* PFB_OPT_TILE_WAVES (a handle's default: 8) */
  int nontemporal;        /* PFB_OPT_NONTEMPORAL */
  int grid;               /* PFB_OPT_GRID */
  int experiment;         /* PFB_OPT_EXPERIMENT */
  int out_aligned16;      /* the output pointer is a multiple of 16 bytes */
  int reserved;
  uint64_t frames;
} pfb_entry_request;
int pfb_plan_entry(const pfb_entry_request* rq, pfb_kernel_entry* out);

/* Diagnostic: throws a C++ exception of the given kind (0 = std::bad_alloc, 1 = std::runtime_error,
 * 2 = a non-std type) INSIDE the guard every entry point runs under and returns what the guard
 * returns (PFB_ERR_NO_MEMORY / PFB_ERR_INTERNAL): proof that nothing thrown crosses the C ABI. */
int pfb_selftest_exception_guard(int kind);

#ifdef __cplusplus
}
#endif
#endif /* PFB_CHANNELIZER_DEV_H */
