// pfb_launch_policy.h -- how a fused plan is launched for one call: schedule, run length, XCD remap, the slab route
// and the slab length, each rule next to the measurement behind it.  Pure host arithmetic over a row of the
// fused-kernel table, the handle's options and the call's frame count -- no device, no HIP -- so launch_frames
// (pfb_api.cpp) and pfb_plan_launch (pfb_channelizer_dev.h, tests/test_plan_table_cpu.py) run the same code.
#pragma once

#include <algorithm>

#include "pfb_channelizer_dev.h"

namespace pfb {

// what the policy may look at besides the plan row and the frame count (pfb_launch_request without its struct_size)
struct LaunchRequest {
  int schedule;                  // PFB_OPT_SCHEDULE, -1 = default
  int frames_per_block;          // PFB_OPT_FRAMES_PER_BLOCK, 0 = default
  int xcd_remap;                 // PFB_OPT_XCD_REMAP, -1 = per schedule
  int64_t slab_frames;           // PFB_OPT_SLAB_FRAMES, 0 = default
  int channel_major, magnitude;  // the handle's layout / PFB_FLAG_MAGNITUDE
  int num_cus;
};

// The report of the fused launch of `frames` frames: what goes into KernelParams (schedule, frames_per_block,
// xcd_remap), the route (by_slabs, slab_frames) and the runs that makes.
inline pfb_launch_report plan_launch(const pfb_fast_plan_desc& plan, const LaunchRequest& rq, uint64_t frames) {
  // Channel-major output of a fused shape is written by the kernel itself (its transposed-tile or plain
  // channel-major instantiation) where the plan has one (channel_major_ok, kChannelMajorOk in pfb_fast.hpp).  The
  // 16-wave plans and the three-pass plans on chunks of 4 or 2 frames -- the defaults of M = 1024, 560, 500 and 250,
  // whose fused stores would be 32- or 16-byte runs per channel -- have none and go by slabs instead: the frame-major
  // kernel fills a scratch slab, a transpose kernel moves it into place (1.5-5x faster than the fused stores on those
  // plans, profiles/r04_channel_major_routes.txt).  A slab must be long enough to fill the chip with runs, so it does
  // not fit the memory-side cache; PFB_OPT_SCHEDULE 9 forces the slabs on any shape, PFB_OPT_SLAB_FRAMES sets their length.
  const bool cm = rq.channel_major != 0;
  const bool forced_fused = rq.schedule == 0 || rq.schedule == 2 || rq.schedule == 8;
  // (A fused route for the team plans -- the team kernel transposing its own tiles through an L2-resident scratch -- was
  // bit-identical but slower than the slabs, 7.4 against 6.4 ms per 2^30 samples at M = 1024, and was removed.)
  const bool by_slabs = cm && (!plan.channel_major_ok || rq.schedule == 9);
  const int c = plan.chunk_frames;
  int fpb = rq.frames_per_block > 0 ? rq.frames_per_block : plan.default_frames_per_block;
  fpb = ((fpb + c - 1) / c) * c;
  int schedule = (rq.schedule >= 0 && rq.schedule != 9) ? rq.schedule : plan.default_schedule;
  int xcd_remap = rq.xcd_remap < 0 ? 1 : rq.xcd_remap;
  if (rq.schedule < 0 && rq.magnitude && plan.magnitude_schedule >= 0 && !cm) {
    schedule = plan.magnitude_schedule;  // fused abs(): magnitudes staged in LDS, sliding runs
  }
  if (cm && !by_slabs)  // fused channel-major: 0 = sliding runs, 2 = tiles, 8 = short runs transposed in LDS, else the kernel's pick
    schedule = forced_fused ? rq.schedule : -1;
  if (schedule == 3 && rq.frames_per_block <= 0) fpb = 24;
  // Team kernels run one workgroup per CU, so their runs are dealt in rounds of num_cus, and a last round that is not
  // full costs a whole round: 683 593 frames of M = 1024 in the tuned 512-frame runs are 5.2 rounds = 6 (0.549 of the
  // roofline), in 672-frame runs 3.97 rounds (0.600).  Unless the caller fixed it, the run length is the call's frames
  // split evenly over k full rounds, k chosen for runs near twice the tuned length (full rounds of 1024-frame runs
  // measured +1.3 % over 512: half the pipeline fills and drains) -- short calls thereby spread over every CU instead
  // of filling a few.  (The slab route sizes its slabs as one 512-frame run per CU: already whole rounds.)
  if (schedule == 6 && rq.frames_per_block <= 0 && !by_slabs && frames > 0) {
    // (plans of <= 8 waves are built for several workgroups per CU, 16 waves in all: their rounds are that much wider)
    const long long slots = (long long)rq.num_cus * std::max(1, 16 / ((plan.threads + 64 * c) / 64)), target = 2ll * fpb;
    const long long k = std::max<long long>(1, ((long long)frames + slots * target / 2) / (slots * target));
    const long long even = ((long long)frames + k * slots - 1) / (k * slots);
    fpb = (int)std::min<long long>(std::max<long long>(even, 2 * c), 4 * target);
  }
  // The other kernels with long runs (a wave pair, a lockstep workgroup or a single wave per run of 128-512 frames): a
  // short call must not leave most of the chip idle -- 2 * 10^7 samples of M = 1024 in 512-frame runs kept 39 of 256 CUs
  // busy (0.105 of the roofline; 0.456 spread over all of them).  When the tuned run length gives fewer runs than the
  // chip holds at once, the runs shrink until it is full (at least one chunk pair each).
  if ((schedule == 0 || schedule == 7 || schedule == 11 || schedule == 13) && rq.frames_per_block <= 0 && !by_slabs &&
      !cm && frames > 0) {
    const int waves = std::max(1, plan.threads / 64);
    const long long per_cu = schedule == 7 ? 6 : schedule == 13 ? 2 : std::max(1, 8 / waves);  // runs resident per CU
    const long long slots = rq.num_cus * per_cu;
    if (((long long)frames + fpb - 1) / fpb < slots) {
      const long long even = ((long long)frames + slots - 1) / slots;
      fpb = (int)std::min<long long>(fpb, std::max<long long>(2 * c, (even + c - 1) / c * c));
    }
  }
  if (schedule == 6 || schedule == 7) fpb = ((fpb + 2 * c - 1) / (2 * c)) * (2 * c);  // these kernels walk chunks in pairs
  if (schedule == 4) {
    if (rq.frames_per_block <= 0) fpb = 64;
    if (rq.xcd_remap < 0) xcd_remap = 0;  // 512-frame workgroups: one dense sweep beats L2 halo hits
  }
  // short sliding runs in dispatch order already sweep the stream as one window: leave them round-robin over the XCDs
  if ((schedule == 0 || schedule == 11) && fpb <= 64 && rq.xcd_remap < 0) xcd_remap = 0;
  // The fixed lengths of schedules 3 and 4 (24, 64) are whole chunks of the plans that have those schedules (c = 8).  A
  // plan without them runs its sliding runs at that length, and an interior run stores whole chunks unconditionally:
  // a run that is no whole number of chunks would write past its end, and past the call's last frame.
  fpb = ((fpb + c - 1) / c) * c;
  pfb_launch_report rep{};
  rep.fused = 1;
  rep.schedule = schedule;
  rep.frames_per_block = fpb;
  rep.xcd_remap = xcd_remap;
  rep.by_slabs = by_slabs ? 1 : 0;
  rep.frames = frames;
  rep.runs = (frames + (uint64_t)fpb - 1) / (uint64_t)fpb;
  if (by_slabs) {
    const int hist_samples = plan.M * plan.P + plan.D;
    long long sf = rq.slab_frames > 0 ? rq.slab_frames : (long long)rq.num_cus * fpb;  // one run per CU
    sf = std::max<long long>(64, (sf + 63) / 64 * 64);
    sf = std::max<long long>(sf, (hist_samples + plan.D - 1) / plan.D + 1);  // a later slab's window reaches back into the input, never into the history
    sf = std::min<long long>(sf, 65535ll * 64);  // the transpose kernel's grid: one row of 64 x 64 tiles per 64 frames
    sf = std::min<long long>(sf, ((long long)frames + 63) / 64 * 64);
    // (tried: two slabs and a side stream, slab k transposed while slab k + 1 is filled -- 6.9 ms instead of 6.4 per 2^30
    // samples at M = 1024: the two kernels slow each other down by more than the overlap buys.  One slab, one stream.)
    rep.slab_frames = (uint64_t)sf;
    // every slab but the last holds sf frames
    const uint64_t per_slab = ((uint64_t)sf + (uint64_t)fpb - 1) / (uint64_t)fpb;
    rep.runs = sf > 0 ? frames / (uint64_t)sf * per_slab + (frames % (uint64_t)sf + (uint64_t)fpb - 1) / (uint64_t)fpb : 0;
  }
  return rep;
}

}  // namespace pfb
