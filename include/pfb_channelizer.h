/*
 * pfb_channelizer.h -- C ABI of the MI355X polyphase-filterbank channelizer.
 *
 * This is the drop-in boundary for the reference's channelizer path.  The
 * reference has no FFI for it: the path is MATLAB script code around MathWorks'
 * dsp.Channelizer.  Each entry point below names the reference lines it
 * replaces (paths relative to /root/reference):
 *
 *   pfb_create            dsp.Channelizer(M) construction
 *                         matlab/channelizer_example.m:29-31
 *                         matlab/create_pdws_channelized.m:31-33
 *                         matlab/generate_channelized_training_iq.m:95-98
 *   pfb_process*          int->complex normalise + (conj) transpose + truncate +
 *                         channelizer(x) + fftshift(.,2)
 *                         matlab/channelizer_example.m:18-23,56,58
 *                         matlab/create_pdws_channelized.m:35-60
 *                         input buffer = what the recorders hold:
 *                         cpp/blade_record_iq_12bit.cpp:268,322 (&iq[FILTER_DELAY])
 *                         cpp/usrp_record_iq_08bit.cpp:179,226
 *   pfb_reset             a fresh dsp.Channelizer per file
 *                         matlab/create_pdws_channelized.m:33
 *   pfb_center_frequencies  centerFrequencies(channelizer, fs)
 *                         matlab/channelizer_example.m:60
 *                         matlab/create_pdws_channelized.m:42
 *   pfb_strerror          bladerf_strerror(status) convention
 *                         cpp/blade_record_iq_12bit.cpp:56-60
 *
 * Conventions follow the recorders: every call returns an int status, 0 = OK,
 * negative = failure (never throws, never aborts); the caller owns sample and
 * output buffers; a handle is used by one thread at a time.
 *
 * Arithmetic:
 *   x[n]   = (I[n] + jQ[n]) / 2^(bit_width-1)
 *   y_k[m] = sum_{n=0}^{MP-1} taps[n] e^{+j2 pi k n/M} x[m D + input_offset - n]
 * computed in fp32 on the GPU as M polyphase branches + an M-point FFT.
 * The handle is stateful like the MATLAB System object: samples from earlier
 * calls are the x[n<0] of later ones, and a call whose length is not a multiple
 * of D carries its tail to the next call.
 *
 * There is NO CPU fallback: without a HIP device every compute entry point
 * returns PFB_ERR_NO_DEVICE.
 */
#ifndef PFB_CHANNELIZER_H
#define PFB_CHANNELIZER_H

#include <stddef.h>
#include <stdint.h>

#include "pfb_iq_packet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PFB_ABI_VERSION 2

typedef enum pfb_status {
  PFB_OK = 0,
  PFB_ERR_BAD_ARG = -1,      /* null pointer, size mismatch, value out of range      */
  PFB_ERR_BAD_FORMAT = -2,   /* unknown .iq marker / sample format / bit width       */
  PFB_ERR_UNSUPPORTED = -3,  /* configuration the library has no kernel for          */
  PFB_ERR_NO_DEVICE = -4,    /* no HIP device / HIP runtime unavailable              */
  PFB_ERR_HIP = -5,          /* a HIP call failed (pfb_last_error_detail has more)   */
  PFB_ERR_NO_MEMORY = -6,
  PFB_ERR_CAPACITY = -7,     /* output buffer smaller than the frames produced       */
  PFB_ERR_INTERNAL = -8,     /* a C++ exception other than bad_alloc was stopped at the ABI   */
  PFB_ERR_COMM = -9          /* the caller's halo-exchange callback (RCCL) reported a failure */
} pfb_status;

typedef enum pfb_sample_format {
  PFB_FMT_INT8_IQ = 0,   /* std::complex<int8_t>  (blade/usrp_record_iq_08bit.cpp)   */
  PFB_FMT_INT16_IQ = 1,  /* std::complex<int16_t> (blade/usrp_record_iq_12bit.cpp)   */
  PFB_FMT_CF32 = 2       /* interleaved float I,Q, already normalised                */
} pfb_sample_format;

typedef enum pfb_output_layout {
  PFB_LAYOUT_FRAME_MAJOR = 0,   /* out[m*M + k]      (row-major F x M)               */
  PFB_LAYOUT_CHANNEL_MAJOR = 1  /* out[k*F + m]      (MATLAB's column-major F x M)   */
} pfb_output_layout;

enum {
  PFB_FLAG_FFTSHIFT = 1u << 0,        /* fftshift(out,2): create_pdws_channelized.m:60 */
  PFB_FLAG_CONJUGATE_INPUT = 1u << 1, /* iq' quirk: channelizer_example.m:23           */
  PFB_FLAG_DEROTATE = 1u << 2,        /* y_k[m] *= e^{-j2 pi k m D/M} (identity if D=M) */
  PFB_FLAG_MAGNITUDE = 1u << 3,       /* fused abs(): `out` receives float32 |y_k[m]| instead of  */
                                      /* complex64 (abs(channelizer(x)), channelizer_example.m:56; */
                                      /* mag = abs(iq), create_pdws_channelized.m:67): half the    */
                                      /* output bytes                                              */
  PFB_FLAG_POWER = 1u << 4            /* with PFB_FLAG_MAGNITUDE: |y_k[m]|^2 instead of |y_k[m]|   */
                                      /* (no square root; what a detector that thresholds power    */
                                      /* wants).  Without PFB_FLAG_MAGNITUDE: PFB_ERR_BAD_ARG      */
};

enum {
  PFB_MEM_HOST = 0,   /* iq/out are host pointers: the library stages them            */
  PFB_MEM_DEVICE = 1  /* iq/out are device pointers on the handle's GPU               */
};

typedef struct pfb_config {
  uint32_t struct_size;        /* = sizeof(pfb_config), for ABI growth               */
  uint32_t num_channels;       /* M  (reference: fs*1e-6, channelizer_example.m:29)  */
  uint32_t taps_per_channel;   /* P  (dsp.Channelizer default 12).  Fewer taps than a    */
                               /* fused shape has run on that shape with zeros appended  */
                               /* (pfb_history_samples reports the padded length)        */
  uint32_t decimation;         /* D: 0 or M = maximally decimated, M/2 = 2x oversampled */
  const float* taps;           /* M*P prototype taps h[n], copied at create          */
  uint32_t sample_format;      /* pfb_sample_format                                  */
  uint32_t bit_width;          /* 8, 12 or 16: scale 2^-(bit_width-1); ignored for CF32 */
  uint32_t output_layout;      /* pfb_output_layout                                  */
  uint32_t flags;              /* PFB_FLAG_*                                         */
  int32_t  input_offset;       /* 0..D-1, or -1 for the default D-1                  */
  int32_t  device_id;          /* HIP device ordinal, -1 = current device            */
} pfb_config;

typedef struct pfb_handle pfb_handle;

/* ---- lifecycle ------------------------------------------------------------ */
int pfb_create(const pfb_config* cfg, pfb_handle** out);
int pfb_destroy(pfb_handle* h);
/* zero the filter state, the carried tail and the frame counter */
int pfb_reset(pfb_handle* h);
/* launch on this hipStream_t from now on (default: the null stream).  Work already queued on the
 * previous stream is ordered in front of whatever the new stream runs next for this handle. */
int pfb_set_stream(pfb_handle* h, void* hip_stream);

/* ---- process -------------------------------------------------------------- */
/* Channelize num_samples complex samples.  `iq` is the recorder's buffer
 * (interleaved I,Q of cfg.sample_format).  Frames produced =
 * floor((carried + num_samples)/D) is written to *frames_out; `out` receives
 * frames*M complex64 values and must hold at least out_capacity_frames frames
 * (PFB_ERR_CAPACITY otherwise, with *frames_out = frames needed and no state
 * change).  With PFB_LAYOUT_CHANNEL_MAJOR the column stride is the number of
 * frames of this call.  Synchronous: results are complete on return. */
int pfb_process(pfb_handle* h, const void* iq, uint64_t num_samples, void* out,
                uint64_t out_capacity_frames, uint64_t* frames_out, uint32_t mem);
/* Same, device pointers only, enqueued on the handle's stream without a host
 * sync.  The input buffer must stay valid until pfb_sync (the state update
 * reads its tail on the stream). */
int pfb_process_async(pfb_handle* h, const void* d_iq, uint64_t num_samples, void* d_out,
                      uint64_t out_capacity_frames, uint64_t* frames_out);
int pfb_sync(pfb_handle* h);
/* Frames a call with num_samples would produce right now. */
int pfb_frames_for(const pfb_handle* h, uint64_t num_samples, uint64_t* frames_out);

/* Channelize one .iq record straight from disk: parse the header (pfb_iq_parse_header, all three
 * formats), check that the payload matches it (the reference asserts length(iq)==numSamples,
 * matlab/convert_my_iq_to_mat.m:102) and that the handle was created for its sample format and
 * bit width, then stream the payload through the GPU in chunks without holding the file in
 * memory.  Replaces convert_my_iq_to_mat.m:40-118 + the load/normalise lines of the channelizer
 * scripts for the common case.  `out` is host memory; a channel-major handle fills one M x frames
 * matrix for the whole record (column stride = the record's frame count).  The handle's state
 * carries over exactly as with pfb_process (call pfb_reset first for a fresh channelizer per file,
 * create_pdws_channelized.m:33). */
int pfb_process_iq_file(pfb_handle* h, const char* path, void* out, uint64_t out_capacity_frames,
                        uint64_t* frames_out, pfb_iq_info* info_out);

/* ---- state (checkpoint/resume, and the multi-GPU halo) --------------------- */
/* History is the raw input samples (cfg.sample_format) that precede the next
 * call: pfb_history_samples() of them.  A time shard on GPU g>0 is primed with
 * the last pfb_history_samples() samples of shard g-1. */
uint64_t pfb_history_samples(const pfb_handle* h);
/* Feed samples into the history without producing output (n may be any size;
 * only the trailing pfb_history_samples() matter).  Carried-tail phase is
 * advanced by n exactly as pfb_process would. */
int pfb_prime(pfb_handle* h, const void* iq, uint64_t num_samples, uint32_t mem);
/* Opaque state blob: history + counters.  Query size with buf == NULL. */
int pfb_get_state(pfb_handle* h, void* buf, size_t* bytes);
int pfb_set_state(pfb_handle* h, const void* buf, size_t bytes);
/* Global index of the next frame (used by PFB_FLAG_DEROTATE); settable so a
 * time shard can start mid-stream. */
int pfb_set_frame_index(pfb_handle* h, uint64_t next_frame);
int pfb_get_frame_index(const pfb_handle* h, uint64_t* next_frame);

/* ---- time-sharded streams: one segment per GPU ------------------------
 * The reference channelizes a whole record in one call (matlab/create_pdws_channelized.m:57); a host
 * that cuts the stream into G contiguous segments, one per GPU, needs exactly one exchange: the last
 * pfb_halo_samples() RAW samples of segment g are the filter state of segment g+1.  The library
 * orchestrates the step and leaves the transport to the caller, so it links no communication library
 * itself: the callback is where a C++ host puts
 *     ncclGroupStart(); ncclSend(d_send, bytes, ncclUint8, send_to, comm, stream);
 *                       ncclRecv(d_recv, bytes, ncclUint8, recv_from, comm, stream); ncclGroupEnd();
 * (examples/sharded_rccl.cpp; sdr_channelizer_amd/sharded.py does the same through torch.distributed).
 * It must ENQUEUE both transfers on `hip_stream` and return without waiting; either side may be absent
 * (rank < 0 and pointer NULL: the first shard of a non-ring stream receives nothing, the last sends
 * nothing).  Return 0 on success; anything else makes the call fail with PFB_ERR_COMM. */
typedef int (*pfb_halo_exchange_fn)(void* user, const void* d_send, void* d_recv, size_t bytes,
                                    int send_to_rank, int recv_from_rank, void* hip_stream);
typedef struct pfb_shard_config {
  uint32_t struct_size;          /* = sizeof(pfb_shard_config)                                    */
  int32_t rank, world;           /* this handle owns segment `rank` of `world`                    */
  uint32_t ring;                 /* 1: rank 0 receives from rank world-1 (the segments of call i+1 */
                                 /* follow those of call i: an endless stream, what bench.py times).  */
                                 /* The last rank then sends its CARRIED state -- the tail of its    */
                                 /* previous segment, zeros after pfb_reset -- not the tail of the   */
                                 /* segment in hand: its send of call i is what rank 0's receive of  */
                                 /* call i is matched with, and rank 0 is one call ahead of it.      */
                                 /* 0: rank 0 continues from the handle's own state                */
  pfb_halo_exchange_fn exchange; /* may be NULL when world == 1                                   */
  void* user;
} pfb_shard_config;
/* Make the handle one shard of a time-sharded stream (world == 1 detaches). */
int pfb_shard_attach(pfb_handle* h, const pfb_shard_config* cfg);
/* Raw samples a shard needs from its predecessor: M*P - 1 - input_offset, i.e. (P-1)*M with the
 * default input_offset D-1 at D = M -- the (taps_per_branch-1)*M overlap and nothing more. */
uint64_t pfb_halo_samples(const pfb_handle* h);
/* The first frames of a segment whose windows reach into the halo: ceil(pfb_history_samples / D). */
uint64_t pfb_shard_head_frames(const pfb_handle* h);
/* Where the predecessor's tail lands (device memory owned by the handle, pfb_halo_samples() samples
 * of cfg.sample_format): what the library passes to the callback as d_recv. */
void* pfb_halo_recv_buffer(pfb_handle* h);
/* Channelize this rank's segment (device pointers; num_samples a multiple of D and at least
 * pfb_history_samples(), carried tail empty).  Enqueued, no host sync:
 *   side stream : the halo exchange (the callback), ordered behind what the handle's stream has queued
 *   main stream : frames [head, F) -- every frame whose window lies inside the segment -- start at
 *                 once; frames [0, head) follow when the halo has landed (one event wait on the GPU).
 * The result is bit-identical to channelizing the whole stream on one device.  The handle's state
 * afterwards is the segment's tail, as after pfb_process.  pfb_sync() also covers the transfers. */
int pfb_process_shard_async(pfb_handle* h, const void* d_segment, uint64_t num_samples, void* d_out,
                            uint64_t out_capacity_frames, uint64_t* frames_out);

/* ---- helpers -------------------------------------------------------------- */
/* centerFrequencies(channelizer, fs).  What order MathWorks' function returns is NOT pinned here
 * (closed toolbox).  matlab/channelizer_example.m:58-66 plots
 * fftshift(out,2) against fc - centerFrequencies(channelizer,fs), which only reads sensibly if the
 * list is already centred and ascending; matlab/create_pdws_channelized.m:42,80 indexes it with the
 * fftshift-ed column either way.  Both orders are offered:
 *   PFB_FREQ_ORDER_FFT       out[k] = [0,1,..,ceil(M/2)-1,-floor(M/2),..,-1]*fs/M  (column k of `out`)
 *   PFB_FREQ_ORDER_CENTERED  out[c] = (c - floor(M/2))*fs/M                        (column c of fftshift(out,2))
 * pfb_center_frequencies is the FFT order (the frequency of UNSHIFTED output column k). */
enum { PFB_FREQ_ORDER_FFT = 0, PFB_FREQ_ORDER_CENTERED = 1 };
int pfb_center_frequencies(uint32_t num_channels, double fs, double* out);
int pfb_center_frequencies_ordered(uint32_t num_channels, double fs, uint32_t order, double* out);
/* Convenience prototype: Kaiser-windowed sinc, M*P taps, cutoff fs/(2M).
 * NOT verified against MathWorks' internal design -- pass your own taps for
 * parity work. */
int pfb_design_prototype(uint32_t num_channels, uint32_t taps_per_channel,
                         double stopband_atten_db, float* taps_out);
const char* pfb_strerror(int status);
/* Text of the most recent HIP failure on this thread ("" if none). */
const char* pfb_last_error_detail(void);
int pfb_abi_version(void);
int pfb_device_count(void);

/* ---- tuning / introspection (stable names, values may grow) ----------------
 * Production knobs only.  The measurement entry points (copy-kernel yardsticks, the exception-guard self test) and the
 * kernel-study options (PFB_OPT_GRID / TILE_WAVES / EXPERIMENT / VARIANT) live in pfb_channelizer_dev.h: same library,
 * same pfb_set_option, not part of what an integrator binds. */
typedef enum pfb_option {
  PFB_OPT_KERNEL = 0,           /* 0 = auto, 1 = force generic kernel, 2 = require fast kernel */
  PFB_OPT_FRAMES_PER_BLOCK = 1, /* run length per workgroup for the fast kernels (0 = default) */
  PFB_OPT_HOST_CHUNK_SAMPLES = 2, /* staging chunk for PFB_MEM_HOST (0 = default)              */
  PFB_OPT_NONTEMPORAL = 3,      /* 1 = nontemporal output stores                               */
  PFB_OPT_PROFILE = 4,          /* 1 = bracket every channelizer kernel launch with HIP events  */
  PFB_OPT_XCD_REMAP = 5,        /* -1 (default) = per schedule, 1 = consecutive runs stay on one XCD, */
                                /* G > 1 = in groups of G workgroups (schedule 3), 0 = off       */
  PFB_OPT_SCHEDULE = 6,         /* fast kernels: -1 (default) = best measured for the kernel; every schedule of a shape gives */
                                /* the same bits.  Frame-major: 0 = one sliding-window run per workgroup, 2 = one chunk per   */
                                /* wave with adjacent chunks grouped into workgroups, 3 = short sliding runs whose halo rows  */
                                /* are shared through LDS, 4 = 3 with the FIR and the FFT on different waves (M = 64), 6 = a  */
                                /* FIR team + an FFT team in one workgroup (M = 1024 / 560), 7 = a FIR wave + an FFT wave per */
                                /* long sliding run, 11 = 0 software-pipelined inside the wave (M = 128 D = 64), 13 = several */
                                /* independent few-wave workgroups per CU (a variant of M = 1024).  Channel-major handles:    */
                                /* 0 / 2 as above, 8 = short runs whose output is transposed in LDS, 9 = frame-major slabs +  */
                                /* a transpose kernel (the default of the M = 1024 / 560 plans).  1, 5, 10, 12: removed.      */
  /* 7 ... 10: pfb_channelizer_dev.h */
  PFB_OPT_SLAB_FRAMES = 11      /* channel-major by slabs (schedule 9): frames per slab, 0 = one run per CU */
} pfb_option;
int pfb_set_option(pfb_handle* h, int option, int64_t value);
/* With PFB_OPT_PROFILE on: durations (ms) of the channelizer kernel launches
 * since the option was set or since the last call of this function, measured
 * by hipEvents recorded on the handle's stream immediately around each launch
 * (oldest first, at most 4096 kept).  Synchronises the stream.  *count receives
 * the number written (<= capacity). */
int pfb_get_kernel_times(pfb_handle* h, float* ms_out, int capacity, int* count);
/* Name of the kernel the last process call launched ("" before the first). */
const char* pfb_last_kernel(const pfb_handle* h);
/* The device the handle lives on (pfb_config.device_id resolved: -1 became the device current at pfb_create). */
int pfb_get_device(const pfb_handle* h, int* device_id);

/* Page-locked host memory for the sample and output buffers of PFB_MEM_HOST calls -- what the
 * recorders would use in place of `new std::complex<std::int16_t>[n]`
 * (cpp/blade_record_iq_12bit.cpp:268).  The host path copies chunk i+1 in while chunk i is
 * transformed and chunk i-1 is copied out; only page-locked buffers let the two PCIe directions
 * really overlap (pageable memory works, at the rate of the runtime's own staging).  NULL on failure. */
void* pfb_host_alloc(size_t bytes);
void pfb_host_free(void* p);

/* ---- channelized PDW extraction ------------------------------------------------
 * Replaces the second half of matlab/create_pdws_channelized.m (lines 64-143): per-channel
 * noise floor = median magnitude (:73), threshold NF*10^(SNR_THRESHOLD/10) (:74-75), the
 * leading/trailing-edge state machine over frames (:85-135), and per pulse the median
 * magnitude (:101), SNR (:105), pulse width (:110), median wrapped phase step -> frequency
 * (:114-122) and the saturation flag (:130-132).  Input is the F x M matrix the channelizer
 * produced (frame-major complex64, already fftshift-ed as in :60), on the GPU or the host.
 * PDWs come back in the reference's order: channels outermost, time within a channel. */
typedef struct pfb_pdw {
  double toa;   /* UTC seconds: (1-based frame index)/fs + sample_start_time (:98)        */
  double freq;  /* Hz (:122)                                                             */
  double pw;    /* seconds (:110)                                                        */
  double snr;   /* dB (:105)                                                             */
  int32_t sat;  /* 0/1 (:130-132)                                                        */
  int32_t bin;  /* 0-based (shifted) column the pulse was found in                       */
  double mag;   /* median magnitude over the pulse: thisAmp (:101; the channelized script
                   does not store it) / pdw.mag of matlab/create_pdws.m:70,96            */
} pfb_pdw;

enum {
  /* reproduce the reference's indexing quirk at :114: phase(toa:jj) linear-indexes COLUMN 1 of the
   * phase matrix whatever channel the pulse is in.  Without the flag the pulse's own column is used. */
  PFB_PDW_MATLAB_QUIRKS = 1u << 0,
  /* `y` is channel-major, y[k*frames + m]: MATLAB's own column-major F x M matrix (what pfb_process
   * writes for a PFB_LAYOUT_CHANNEL_MAJOR handle).  Transposed once into device scratch. */
  PFB_PDW_CHANNEL_MAJOR = 1u << 1,
  /* fc_chan = fc + binFreqs(bin) (:80) with binFreqs in FFT order (PFB_FREQ_ORDER_FFT) indexed by the
   * fftshift-ed column -- what the script computes IF MathWorks' centerFrequencies returns the unshifted
   * list; every pulse's freq is then half the band away from its channel.  Unpinned (see
   * pfb_center_frequencies): the default is the column's true centre frequency, which is also what the
   * script computes if centerFrequencies returns the centred list. */
  PFB_PDW_BINFREQ_UNSHIFTED = 1u << 2
};

/* fs_in: sample rate BEFORE decimation; the frame rate used is fs_in/decimation (:62).
 * noise_floor_out (optional, M doubles): the per-channel medians.  *count receives the number
 * of pulses found even when it exceeds capacity (only `capacity` are written).
 * mem: PFB_MEM_HOST / PFB_MEM_DEVICE for `y`; `out` and `noise_floor_out` are host memory. */
int pfb_pdw_extract(const void* y, uint64_t frames, uint32_t num_channels, uint32_t decimation,
                    double fs_in, double fc, double sample_start_time, double snr_threshold_db,
                    uint32_t flags, pfb_pdw* out, uint64_t capacity, uint64_t* count,
                    double* noise_floor_out, uint32_t mem, int32_t device_id, void* hip_stream);
/* ---- raw (un-channelized) PDW extraction -----------------------------------------
 * Replaces matlab/create_pdws.m:30-105: the same extraction on the recorder stream itself.
 * x = (I + jQ) / 2^(bit_width-1) (:30-33); ONE noise floor = median |x| (:44); a pulse starts at
 * |x| >= NF*10^(snr_threshold_db/10) (:45-46,57) and ends at |x| <= NF*10^(trailing_threshold_db/10)
 * (:47,63) -- the script uses 18 and 3 dB; trailing must not exceed leading.  Per pulse: toa (:67),
 * mag (:70), snr (:74), pw (:79), freq = fc + fs/(360/median wrapped phase step) (:83-91), sat
 * (:100-102); bin is 0.  `iq` is interleaved I,Q in `sample_format` (PFB_FMT_*), host or device per
 * `mem`; fs is the sample rate; noise_floor_out (optional) receives the one median.  *count receives
 * the number of pulses found even when it exceeds capacity. */
int pfb_pdw_extract_raw(const void* iq, uint64_t num_samples, uint32_t sample_format, uint32_t bit_width,
                        double fs, double fc, double sample_start_time, double snr_threshold_db,
                        double trailing_threshold_db, pfb_pdw* out, uint64_t capacity, uint64_t* count,
                        double* noise_floor_out, uint32_t mem, int32_t device_id, void* hip_stream);
/* One iteration of the loop in matlab/create_pdws_channelized.m:22-143 -- load a record, channelize
 * it, fftshift (the handle's PFB_FLAG_FFTSHIFT), extract its PDWs -- in one call: the payload is
 * streamed to the GPU as in pfb_process_iq_file, the F x M channel matrix stays in device memory
 * (scratch kept on the handle, freed with it) and only the PDWs come back.  fs, fc and the sample
 * start time are the record's (sampleRateSps, frequencyHz, sampleStartTime: the values
 * convert_my_iq_to_mat.m stores in the .mat the script loads).  The handle must be frame-major with
 * complex output and match the record's format and bit width; its state carries over as with
 * pfb_process (pfb_reset first for a fresh channelizer per file, :33).  Remaining arguments as in
 * pfb_pdw_extract. */
int pfb_pdw_from_iq_file(pfb_handle* h, const char* path, double snr_threshold_db, uint32_t flags,
                         pfb_pdw* out, uint64_t capacity, uint64_t* count, double* noise_floor_out,
                         pfb_iq_info* info_out);
/* One iteration of the loop in matlab/create_pdws.m (load a record, :30-105 on its raw stream):
 * the payload goes to the device through page-locked chunks, pfb_pdw_extract_raw runs there, the PDWs
 * come back.  fs, fc, bit width and start time are the record's. */
int pfb_pdw_raw_from_iq_file(const char* path, double snr_threshold_db, double trailing_threshold_db,
                             pfb_pdw* out, uint64_t capacity, uint64_t* count, double* noise_floor_out,
                             pfb_iq_info* info_out, int32_t device_id);
/* Text of the most recent HIP failure inside pfb_pdw_extract on this thread. */
const char* pfb_pdw_last_error_detail(void);
/* How the last pfb_pdw_extract on this thread found the noise floors: 1 = sampled bracket + one
 * pass that also produced the edge masks, 4 = the same but the masks needed their own pass (too many
 * samples near the threshold, or a median at the very edge of its bracket), 2 = full radix select
 * (short input), 3 = the bracket check failed (heavily tied data) and the full radix select ran
 * after it.  All give the exact medians and edges; diagnostic only. */
int pfb_pdw_last_noise_floor_path(void);
/* pfb_pdw_extract keeps its device scratch between calls (grow-only, per device; calls are
 * serialised on it).  This frees it: device_id >= 0 for one device, < 0 for all. */
int pfb_pdw_release_workspace(int32_t device_id);

/* ---- dwell analysis and event prediction -------------------------------------------------------
 * The last layer of the reference: capture a dwell, find its pulses, fit the SNR-vs-TOA parabola, schedule
 * the next capture (matlab/predict_event.m:53-138, cpp/usrp_predict_event.cpp:285-375), plus the gain finders'
 * saturation scan (cpp/usrp_find_max_unsaturated_gain.cpp:146, cpp/blade_find_max_unsaturated_gain.cpp:268).
 * x = (I + jQ) / 2^(bit_width-1) (predict_event.m:48-51; cf32 as is).  With i0 and j the 0-based leading and
 * trailing sample of a pulse, both statistics share:
 *   noise floor NF, threshold NF*10^(snr_threshold_db/10) (m:64-66, cpp:289-291); leading edge |x| >= thr,
 *   trailing edge |x| <= thr (m:76,82, cpp:306,316); snr = 10*log10(amp/NF) (m:93, cpp:329); pw = (j - i0)/fs
 *   (m:98); sat from the samples strictly inside the pulse with |I| or |Q| >= 0.9999 (m:118, cpp:336); bin = 0;
 *   a pulse still active at the end of the buffer gives no PDW; *count is the number found, even beyond
 *   `capacity` (only `capacity` are written).
 * PFB_DWELL_STAT_MEDIAN (predict_event.m:64-121): NF = median |x| (:64), amp = median of |x| over i0..j
 *   inclusive (:89), toa = (i0+1)/fs + sample_start_time (:86, 1-based), freq as create_pdws.m (:102-110).
 *   Bit-identical to pfb_pdw_extract_raw with trailing_threshold_db == snr_threshold_db: it is that code.
 * PFB_DWELL_STAT_MEAN (usrp_predict_event.cpp:287-343): NF = mean |x| (:288-289), amp = (sum of |x_i| over
 *   i0 <= i < j)/(j - i0) (:311,334,325: the trailing sample is not in the sum), toa = i0/fs + sample_start_time
 *   (:321, 0-based), freq = fc + fs/(360/median wrapped phase step of i0..j) as the other extractors compute it
 *   (the C++ loop has none), or NaN with PFB_DWELL_SKIP_FREQ.  Arithmetic is float64: the reference's float32
 *   cwiseAbs()/mean() (:288-289) is NOT reproduced.  The sums are taken in a fixed order, so the same buffer
 *   gives the same bits on every call.
 * pfb_dwell_stats comes from one pass over the buffer; with full = 2^(bit_width-1):
 *   saturated_components  the I and Q components c (raw integers, compared in double) with
 *                         c <= sat_fraction*(-full) or c >= sat_fraction*(full-1): the gain finders' test; for
 *                         cf32 the limits are -sat_fraction and +sat_fraction
 *   mean_mag, peak_mag    mean and max of |x|; peak_mag is what predict_event.m:53 gates on (> 0.9)
 *   peak_component        max of |I|/full, |Q|/full
 *   noise_floor, threshold the ones the edges used; pulses = *count
 *   any_pulse_saturated   OR of sat over the PDWs written (the first min(*count, capacity))
 * `iq` is host or device memory per cfg->mem; `out` and `stats` are host memory.  Every argument is validated
 * before the device is touched: PFB_ERR_BAD_ARG for a null cfg / iq / count / stats (or out with capacity > 0),
 * a wrong struct_size, num_samples < 2, bit_width outside 1..16 for the integer formats, an unknown
 * sample_format, statistic, flag or mem, sat_fraction outside [0, 1], a non-finite fs or threshold; then
 * PFB_ERR_NO_DEVICE without a HIP device.  Shares the PDW extractors' device scratch
 * (pfb_pdw_release_workspace) and error text (pfb_pdw_last_error_detail). */
enum { PFB_DWELL_STAT_MEAN = 0, PFB_DWELL_STAT_MEDIAN = 1 };
enum { PFB_DWELL_SKIP_FREQ = 1u << 0 };   /* freq = NaN, no phase work: the live loop reads toa and snr only */

typedef struct pfb_dwell_config {
  uint32_t struct_size;    /* = sizeof(pfb_dwell_config)                                        */
  uint32_t sample_format;  /* pfb_sample_format                                                 */
  uint32_t bit_width;      /* 1..16: scale 2^-(bit_width-1); ignored for CF32                   */
  uint32_t statistic;      /* PFB_DWELL_STAT_*                                                  */
  uint32_t flags;          /* PFB_DWELL_SKIP_FREQ (MEAN only; MEDIAN ignores it)                */
  uint32_t mem;            /* PFB_MEM_HOST / PFB_MEM_DEVICE for `iq`                            */
  int32_t device_id;       /* HIP device ordinal, -1 = current device                           */
  double fs, fc, sample_start_time;
  double snr_threshold_db; /* both sources: 20 (m:65, cpp:290)                                  */
  double sat_fraction;     /* gain finders: 0.98; 0 = 0.98                                      */
} pfb_dwell_config;

typedef struct pfb_dwell_stats {
  uint64_t num_samples, saturated_components, pulses;
  double mean_mag, peak_mag, peak_component;
  double noise_floor, threshold;
  int32_t any_pulse_saturated, reserved;
} pfb_dwell_stats;

int pfb_dwell_analyze(const pfb_dwell_config* cfg, const void* iq, uint64_t num_samples, pfb_pdw* out,
                      uint64_t capacity, uint64_t* count, pfb_dwell_stats* stats, void* hip_stream);
/* One record from disk: its header supplies sample format, bit width, fs, fc and start time (overriding cfg's);
 * the payload is loaded as pfb_pdw_raw_from_iq_file loads it; cfg->mem is ignored. */
int pfb_dwell_from_iq_file(const char* path, const pfb_dwell_config* cfg, pfb_pdw* out, uint64_t capacity,
                           uint64_t* count, pfb_dwell_stats* stats, pfb_iq_info* info_out);
/* Host only.  Least-squares quadratic of snr against toa (predict_event.m:125-130 polyfit,
 * usrp_predict_event.cpp:28-52 householderQr), solved by Householder QR in double on tau = toa - toa[0]: raw
 * UTC seconds squared are not representable well enough, and the peak is translation-invariant.
 * coef = [p0, p1, p2] of p0 + p1*tau + p2*tau^2; *t_peak = toa[0] - p1/(2*p2) (m:129, cpp:51), *snr_peak the
 * parabola there (m:130).  n < 3 or a null pointer: PFB_ERR_BAD_ARG.  A fit that is not concave or not finite
 * (p2 >= 0, rank-deficient abscissae): PFB_ERR_UNSUPPORTED with coef filled.  The reference's own gate,
 * toaList.size() > 10 (cpp:348), is the caller's. */
int pfb_event_fit(const pfb_pdw* pdws, uint64_t n, double* t_peak, double* snr_peak, double coef[3]);
/* Host only.  Next event from the event times so far.  convention 0 (predict_event.m:134-138): next = last +
 * median(diff) with MATLAB's median (mean of the middle two for an even count), *have_next = 0 when n < 2 (the
 * script's hard-coded first period is the caller's business).  convention 1 (usrp_predict_event.cpp:354-372): only
 * when n > 5, the median is sorted_diff[size/2].  Other conventions: PFB_ERR_BAD_ARG. */
int pfb_event_next(const double* event_times, uint64_t n, uint32_t convention, double* next, int32_t* have_next);


/* ---- short-time Fourier transform of an I/Q stream --------------------------------------------
 * Replaces the spectrogram lines of the reference scripts:
 *   matlab/spectrogram_my_iq.m:105-115   [s,f,t] = stft(iq,fs,'Window',hamming(768),'OverlapLength',0)
 *                                         on iq = (I + jQ)/2^(bitWidth-1) (no conjugate), abs(s).^2 plotted
 *   matlab/generate_pulsed_iq.m:105       spectrogram(iq,1024,0,1024,Fs,'centered','yaxis'): PSD in dB
 * Arithmetic, with w[0..L-1] the caller's window, H the hop and nfft >= L the FFT length:
 *   frame m covers x[mH .. mH+L-1]; N samples give F = floor((N-L)/H) + 1 frames (0 if N < L): partial
 *   windows are never produced.
 *   s[r,m] = sum_{n<L} w[n] x[mH+n] e^{-j 2 pi k_r n / nfft}       (phase origin: the frame's first sample)
 *   PFB_STFT_CENTERED  k_r = r - nfft/2 + 1 (even nfft: (-pi, pi], Nyquist last), r - (nfft-1)/2 (odd):
 *                      stft's default 'centered' -- NOT fftshift, which differs by one row at even nfft
 *   PFB_STFT_TWOSIDED  k_r = r (FFT order)
 * Output out[m*nfft + r]: MATLAB's column-major nfft x F matrix s.  PFB_STFT_POWER stores scale*|s|^2,
 * PFB_STFT_DB 10*log10(scale*|s|^2 + db_floor) (float32); PFB_STFT_COMPLEX stores s (complex64).
 * Unpinned (closed toolbox; pfb_stft_axes and DESIGN.md section 11 keep each in one place):
 *   - the time axis: t_m = (m*H + L/2)/fs, the segment centre (spectrogram's colindex-1 + nwind/2);
 *   - stft's default FFTLength when only 'Window' is given: fft_length = 0 means nfft = L;
 *   - spectrogram's PSD scale 1/(fs*sum w^2) and the eps its plot adds: the caller's scale / db_floor.
 * The handle is stateful: it carries the samples from the start of the next frame (fewer than L), so any
 * cutting of a stream into calls gives the same bits as one call. */
enum { PFB_STFT_COMPLEX = 0, PFB_STFT_POWER = 1, PFB_STFT_DB = 2 };
enum { PFB_STFT_CENTERED = 0, PFB_STFT_TWOSIDED = 1 };
enum { PFB_STFT_KERNEL_AUTO = 0, PFB_STFT_KERNEL_GENERIC = 1, PFB_STFT_KERNEL_FUSED = 2 };

typedef struct pfb_stft_config {
  uint32_t struct_size;    /* = sizeof(pfb_stft_config)                                              */
  uint32_t window_length;  /* L >= 1                                                                 */
  uint32_t hop;            /* H = L - OverlapLength, 1 <= H <= L; 0 = L (no overlap)                 */
  uint32_t fft_length;     /* nfft, L <= nfft <= 4096 (zero padding); 0 = L                          */
  const float* window;     /* L coefficients, copied at create                                       */
  uint32_t sample_format;  /* pfb_sample_format                                                      */
  uint32_t bit_width;      /* 8, 12 or 16: scale 2^-(bit_width-1); ignored for CF32                  */
  uint32_t output;         /* PFB_STFT_COMPLEX / POWER / DB                                          */
  uint32_t freq_order;     /* PFB_STFT_CENTERED (stft's default) / PFB_STFT_TWOSIDED                 */
  double scale;            /* power and dB: multiplies |s|^2; 0 = 1                                  */
  double db_floor;         /* dB: added before log10 (>= 0; 0 gives -inf for an all-zero bin)       */
                           /* Both are applied in float32: nonzero values outside [FLT_MIN, FLT_MAX] */
                           /* are PFB_ERR_BAD_ARG                                                   */
  uint32_t kernel;         /* PFB_STFT_KERNEL_*: FUSED = fused kernel or PFB_ERR_UNSUPPORTED         */
  int32_t device_id;       /* HIP device ordinal, -1 = current device                                */
} pfb_stft_config;

typedef struct pfb_stft_handle pfb_stft_handle;

/* Lifecycle as pfb_create / pfb_destroy / pfb_reset / pfb_set_stream.  Every argument is validated before
 * the device is touched: PFB_ERR_BAD_ARG, PFB_ERR_BAD_FORMAT, PFB_ERR_UNSUPPORTED (nfft > 4096, or FUSED
 * asked for an nfft without a fused kernel), then PFB_ERR_NO_DEVICE without a HIP device. */
int pfb_stft_create(const pfb_stft_config* cfg, pfb_stft_handle** out);
int pfb_stft_destroy(pfb_stft_handle* h);
int pfb_stft_reset(pfb_stft_handle* h);
int pfb_stft_set_stream(pfb_stft_handle* h, void* hip_stream);
/* Transform num_samples samples; frames = what pfb_stft_frames_for reports, written to *frames_out.
 * `out` must hold out_capacity_frames * nfft values (PFB_ERR_CAPACITY otherwise, with *frames_out = the
 * frames needed and no state change).  mem = PFB_MEM_HOST / PFB_MEM_DEVICE.  Synchronous.  Device pointers must be
 * aligned to one sample (iq) and one output element (out): PFB_ERR_BAD_ARG otherwise.  Host pointers are staged
 * as pfb_process stages them (chunks of at most 64 MiB per side, copy-in, transform and copy-out overlapped;
 * page-locked buffers from pfb_host_alloc overlap the two PCIe directions). */
int pfb_stft_process(pfb_stft_handle* h, const void* iq, uint64_t num_samples, void* out,
                     uint64_t out_capacity_frames, uint64_t* frames_out, uint32_t mem);
/* Same, device pointers, enqueued on the handle's stream without a host sync. */
int pfb_stft_process_async(pfb_stft_handle* h, const void* d_iq, uint64_t num_samples, void* d_out,
                           uint64_t out_capacity_frames, uint64_t* frames_out);
int pfb_stft_sync(pfb_stft_handle* h);
int pfb_stft_frames_for(const pfb_stft_handle* h, uint64_t num_samples, uint64_t* frames_out);
/* One .iq record from disk (header checked as in pfb_process_iq_file, format and bit width against the
 * handle), streamed as pfb_process_iq_file streams it: chunks of 2^24 samples read into page-locked buffers
 * while the previous chunk goes through the host staging above; `out` is host memory. */
int pfb_stft_process_iq_file(pfb_stft_handle* h, const char* path, void* out, uint64_t out_capacity_frames,
                             uint64_t* frames_out, pfb_iq_info* info_out);
/* Host-only axes: f_out[r] = k_r*fs/nfft (nfft values), t_out[m] = ((first_frame+m)*H + L/2)/fs (frames
 * values).  Either pointer may be NULL. */
int pfb_stft_axes(uint32_t fft_length, uint32_t window_length, uint32_t hop, double fs, uint32_t freq_order,
                  uint64_t first_frame, uint64_t frames, double* f_out, double* t_out);
/* Name of the kernel the last process call launched ("" before the first). */
const char* pfb_stft_last_kernel(const pfb_stft_handle* h);
/* The device the handle lives on (pfb_stft_config.device_id resolved, as pfb_get_device). */
int pfb_stft_get_device(const pfb_stft_handle* h, int* device_id);

/* ---- pulse-train source -----------------------------------------------------------------------------
 * Replaces the reference's signal source:
 *   matlab/generate_pulsed_iq.m:12-19,27-77    rectangular pulses of PW every PRI on a carrier whose phase restarts at
 *                                              every pulse; LFM sweep (:43-47), Barker-13 chips (:33-40,49-59), only
 *                                              pulses that fit the record (:67)
 *   matlab/generate_training_iq.m:34-62,95-98  the same train from a random start index, phase from zero (:44-48),
 *                                              int16(x*2^15) (:97-98)
 *   matlab/generate_training_iq.m:107-127      the hand-written format-1 record (pfb_synth_write_iq_file)
 * The stream is a function from the global sample index i (uint64) to a value, in integers only, so the device, the
 * host and any cutting of the stream into calls give the same bits; it is sdr_channelizer_amd/synth.py's counter-based
 * benchmark stream with the scripts' switches added.  With full = 2^(bit_width-1), derived once on the host in double
 * with round-half-even (pfb_synth_describe reports them):
 *   chip, pw (Barker)  chip = max(round(pw/13), 1), pw <- 13*chip             (generate_pulsed_iq.m:33-40)
 *   fcw                llrint(f0/fs * 2^32) mod 2^32                          carrier, turns per sample in 2^-32
 *   dcw                llrint(ldexp((lfm_extent_hz/(pw-1))/fs, 64)) mod 2^64  sweep step per sample (0 when pw == 1)
 *   noise_gain         llrint(noise_sigma * full * 2^20 / sqrt(4*(65536^2-1)/12))
 *   tab[j]             llrint(amplitude * full * 2^20 * cos(2 pi j / 65536)), j = 0..65535
 *   barker_offset      llrint(fmod(90/(2 pi), 1) * 2^32): the script adds +-90 to a phase in RADIANS (:50-58,61);
 *                      2^30 (90 degrees) with PFB_SYNTH_BARKER_DEGREES
 * Per sample: rel = i - first_pulse (off when negative), k = rel mod period, s = i - k; the sample is ON iff k < pw and
 * (record_samples == 0 or s + 1 + pw < record_samples: the script's (idx+numSamplesForPw) < length(mag) with its
 * 1-based idx).  kk = k + 1 (the cumsum phase of generate_pulsed_iq.m:45), or k with PFB_SYNTH_PHASE_FROM_ZERO
 * (freq_phi(1) = 0, generate_training_iq.m:44-48); T = k(k+1)/2;
 *   ph = (kk*fcw + ((T*dcw mod 2^64) >> 32) [+ Barker: + barker_offset or + 2^32 - barker_offset by the code of chip
 *        min(k/chip, 12)]) mod 2^32;  ci = ph >> 16, si = (ci - 16384) & 65535
 *   noise (per component, lane 0 = I, 1 = Q): base = lo32(i) ^ (hi32(i)*0x9E3779B1 mod 2^32) ^ seed,
 *        a = mix32(base ^ (0x68E31DA4*(2*lane+1) mod 2^32)), b = mix32(a ^ 0x5BD1E995),
 *        noise = (a & 65535) + (a >> 16) + (b & 65535) + (b >> 16) - 2*65535  (Irwin-Hall, sigma 37837.2 counts)
 *   v = tab[ci or si]*on + noise*noise_gain                                   (2^-20 LSB fixed point)
 *   integer formats: clamp((v + 2^19) >> 20, -full, full-1), round half up; with PFB_SYNTH_ROUND_MATLAB half away from
 *        zero, -((-v + 2^19) >> 20) for v < 0: MATLAB's int16() (generate_training_iq.m:97-98)
 *   PFB_FMT_CF32: (float)((double)v * 2^-(20 + bit_width - 1)), no clamp
 * Against the float64 scripts: the phase of an ON sample agrees with theirs to 3.4e-6 rad (the 32-bit fcw); the
 * resolution that matters is the 16-bit table index, 9.6e-5 rad.
 * Every argument is validated before the device is touched.  PFB_ERR_BAD_ARG: null pointers, a wrong struct_size,
 * not 1 <= pulse_samples <= period_samples < 2^31 (after the Barker adjustment too), amplitude outside [0, 2],
 * noise_sigma outside [0, 1], fs <= 0, a non-finite double, |f0/fs| > 2^20, |lfm step/fs| >= 0.5, unknown flag bits,
 * PFB_SYNTH_BARKER_DEGREES without PFB_SYNTH_BARKER13, start + num_samples overflowing, an output pointer not aligned
 * to one sample.  PFB_ERR_BAD_FORMAT: an unknown sample format, bit_width outside 2..8 (int8) or 2..16 (int16; cf32,
 * where it only scales the table), a cf32 handle or a format-1 record from an int8 handle asked of
 * pfb_synth_write_iq_file.  Then PFB_ERR_NO_DEVICE without a HIP device. */
enum {
  PFB_SYNTH_BARKER13 = 1u << 0,         /* BARKER_13 = true, generate_pulsed_iq.m:17                  */
  PFB_SYNTH_BARKER_DEGREES = 1u << 1,   /* chips of +-90 degrees instead of the script's +-90 radians */
  PFB_SYNTH_PHASE_FROM_ZERO = 1u << 2,  /* generate_training_iq.m:44-48                               */
  PFB_SYNTH_ROUND_MATLAB = 1u << 3      /* int16(): half away from zero                               */
};

typedef struct pfb_synth_config {
  uint32_t struct_size;     /* = sizeof(pfb_synth_config)                                        */
  uint32_t sample_format;   /* pfb_sample_format of the output                                   */
  uint32_t bit_width;       /* full scale 2^(bit_width-1)                                        */
  uint32_t flags;           /* PFB_SYNTH_*                                                       */
  uint32_t pulse_samples;   /* pw: round(fs*PW), generate_training_iq.m:37                       */
  uint32_t period_samples;  /* pri: round(fs*PRI), :38                                           */
  uint32_t seed;            /* of the noise                                                      */
  int32_t device_id;        /* HIP device ordinal, -1 = current device                           */
  uint64_t first_pulse;     /* index of the first pulse's first sample (startIdx, :24-26,40)     */
  uint64_t record_samples;  /* length(mag) of the fit rule; 0 = an endless stream                */
  double fs, f0;            /* sample rate and carrier (f / f_start), Hz                         */
  double lfm_extent_hz;     /* LFM_EXTENT, generate_pulsed_iq.m:18: f_stop - f_start             */
  double amplitude;         /* of an ON sample, in full scales (the scripts: 1)                  */
  double noise_sigma;       /* per component, in full scales (the scripts: 0)                    */
} pfb_synth_config;

typedef struct pfb_synth_params {  /* what the host derived: host only, needs no device */
  uint32_t pulse_samples;          /* after the Barker adjustment */
  uint32_t chip_samples;           /* 0 without PFB_SYNTH_BARKER13 */
  uint32_t fcw, barker_offset;
  uint64_t dcw;
  int64_t noise_gain;
} pfb_synth_params;

typedef struct pfb_synth_handle pfb_synth_handle;

/* Host only: validate cfg and report the derived integers; table_out (65536 values, or NULL) receives tab. */
int pfb_synth_describe(const pfb_synth_config* cfg, pfb_synth_params* out, int64_t* table_out);
/* The handle owns the table in device memory, and holds no stream position: every call names its own. */
int pfb_synth_create(const pfb_synth_config* cfg, pfb_synth_handle** out);
int pfb_synth_destroy(pfb_synth_handle* h);
int pfb_synth_set_stream(pfb_synth_handle* h, void* hip_stream);  /* as pfb_set_stream */
/* Samples start .. start + num_samples - 1 of the stream into `out`: interleaved I,Q of cfg.sample_format, aligned to
 * one sample.  mem = PFB_MEM_DEVICE: one kernel on the handle's stream, complete on return.  PFB_MEM_HOST: generated
 * into page-locked chunks and copied out. */
int pfb_synth_generate(pfb_synth_handle* h, uint64_t start, uint64_t num_samples, void* out, uint32_t mem);
/* Same, device pointer, enqueued on the handle's stream without a host sync. */
int pfb_synth_generate_async(pfb_synth_handle* h, uint64_t start, uint64_t num_samples, void* d_out);
int pfb_synth_sync(pfb_synth_handle* h);
int pfb_synth_get_device(const pfb_synth_handle* h, int* device_id);
/* Write samples start .. start + num_samples - 1 as one .iq record: the header (pfb_iq_serialize_header), then the
 * payload, generated in chunks and never held whole in memory.  file_format 1 is the record
 * generate_training_iq.m:107-127 writes (int16 handles only: the script writes 16-bit), 3 the recorders'.
 * header_fields NULL: link speed 1 (format 1) or 0 (format 3), frequency 0, bandwidth = sample rate = fs, gain 0,
 * board "simulated", start time 0; otherwise its fields, with the marker, numSamples and bitWidth set by the library
 * (bitWidth = cfg.bit_width; the script's own record is bit_width 16).  fs must fit a uint32. */
int pfb_synth_write_iq_file(pfb_synth_handle* h, const char* path, int file_format, uint64_t start,
                            uint32_t num_samples, const pfb_iq_packet* header_fields);

/* ---- magnitude / phase traces and plot envelopes ------------------------------------------------------
 * Replaces the arithmetic of the reference's plotters (drawing stays with the caller):
 *   matlab/plot_my_iq.m:105-108   iq = double(iq)/2^(bitWidth-1); iq = iq(1,:) + 1j*iq(2,:)
 *   matlab/plot_my_iq.m:110-111   mag = abs(iq); phase = rad2deg(angle(iq))            (plotted at :122,129)
 *   the same lines of generate_training_iq.m and generate_channelized_training_iq.m:68-91
 * Per sample, with full = 2^(bit_width-1):
 *   integer formats  u = I^2 + Q^2 as an exact unsigned integer (u <= 2^31, reached by (-32768,-32768): it does not
 *                    fit an int32); power p = u * 2^-(2(bit_width-1))
 *   PFB_FMT_CF32     p = (double)I*(double)I + (double)Q*(double)Q; the products are exact in double, so contraction
 *                    cannot change the result.  Inputs must be finite: a non-finite sample may leave the fields of its
 *                    bin unspecified, and never causes a fault or an access outside the buffers.
 * Envelope: the stream is cut into bins of bin_samples = B consecutive samples, counted from the handle's origin (0
 * after create / reset); pfb_trace_flush starts a new grid at the next sample.  Each bin gives one pfb_trace_bin.
 *   integer formats  everything is integer work: min, max and first-index argmax of u, S = sum of u in uint64
 *                    (B <= 2^31 keeps S < 2^63), converted at the very end: power_min/max = (double)u * scale,
 *                    power_mean = ((double)S / (double)count) * scale, scale = 2^-(2(bit_width-1)).  Every field is
 *                    therefore the same bits under any cutting of the stream into calls, on any pointer alignment, and
 *                    whether the samples come from device memory, host memory or a file.
 *   PFB_FMT_CF32     power_min, power_max and peak_* are exact selections with the same guarantees.  power_mean is a
 *                    double sum taken without floating-point atomics in an order fixed by the call's lengths and its
 *                    pointer's alignment to 16 bytes: the same call gives the same bits every time, another cutting
 *                    may change the last bits.
 * Magnitudes and the peak's phase are the host's in double -- sqrt(power_*), atan2(peak_q, peak_i): one value per bin.
 * No atan2 and no sqrt run on the device for an envelope.
 * Full-rate trace of a stretch (pfb_trace_samples): mag[n] = sqrt(p) and phase_deg[n] = atan2(Q, I)*180/pi, both
 * float32 (mag within 1 ulp of the double value).  Stateless: it reads no carried bin and moves no origin.
 * Every argument is validated before the device is touched.  PFB_ERR_BAD_ARG: null pointers, a wrong struct_size,
 * bin_samples outside 1 .. 2^31, any flag bit (none is defined), an unknown mem, a device iq not aligned to one sample,
 * out not aligned to 8 bytes (mag / phase_deg: to 4).  PFB_ERR_BAD_FORMAT: an unknown sample format, bit_width outside
 * 1..8 (int8) or 1..16 (int16; ignored for cf32).  Then PFB_ERR_NO_DEVICE without a HIP device. */
typedef struct pfb_trace_bin {
  uint64_t peak_sample;   /* global index of the FIRST sample of the bin holding the largest power   */
  double power_min, power_max, power_mean;   /* of p over the bin's samples                           */
  float peak_i, peak_q;   /* that sample's components, normalised (int * 2^-(bit_width-1): exact)     */
  uint32_t count;         /* samples in the bin: B, fewer only for the bin pfb_trace_flush returns    */
  uint32_t reserved;      /* 0 */
} pfb_trace_bin;

typedef struct pfb_trace_config {
  uint32_t struct_size;    /* = sizeof(pfb_trace_config)                 */
  uint32_t sample_format;  /* pfb_sample_format                          */
  uint32_t bit_width;      /* full scale 2^(bit_width-1)                 */
  uint32_t bin_samples;    /* B, 1 .. 2^31                               */
  uint32_t flags;          /* 0                                          */
  int32_t device_id;       /* HIP device ordinal, -1 = current device    */
} pfb_trace_config;

typedef struct pfb_trace_handle pfb_trace_handle;

/* Lifecycle as pfb_stft_*.  The handle holds the stream position and, on the device, the bin a call left open. */
int pfb_trace_create(const pfb_trace_config* cfg, pfb_trace_handle** out);
int pfb_trace_destroy(pfb_trace_handle* h);
int pfb_trace_reset(pfb_trace_handle* h);   /* origin back to 0, no open bin */
int pfb_trace_set_stream(pfb_trace_handle* h, void* hip_stream);
int pfb_trace_sync(pfb_trace_handle* h);
int pfb_trace_get_device(const pfb_trace_handle* h, int* device_id);
/* The bins the next call of num_samples samples completes. */
int pfb_trace_bins_for(const pfb_trace_handle* h, uint64_t num_samples, uint64_t* bins_out);
/* The records of the bins these samples complete, to `out` (room for capacity_bins); *bins_out = their number.
 * PFB_ERR_CAPACITY sets *bins_out to the number needed and changes no state.  mem: iq and out are both host pointers
 * (PFB_MEM_HOST, staged as pfb_stft_process stages them) or both device pointers (PFB_MEM_DEVICE).  Synchronous. */
int pfb_trace_envelope(pfb_trace_handle* h, const void* iq, uint64_t num_samples, pfb_trace_bin* out,
                       uint64_t capacity_bins, uint64_t* bins_out, uint32_t mem);
/* Same, device pointers, enqueued on the handle's stream without a host sync (bins longer than 4096 samples use a
 * device scratch that grows with the longest call so far: a call that grows it waits for the device). */
int pfb_trace_envelope_async(pfb_trace_handle* h, const void* d_iq, uint64_t num_samples, pfb_trace_bin* d_out,
                             uint64_t capacity_bins, uint64_t* bins_out);
/* The open bin, if any, to host memory (*have = 0 / 1; its count < B), and a new bin grid from the next sample. */
int pfb_trace_flush(pfb_trace_handle* h, pfb_trace_bin* out_host, int32_t* have);
/* mag and phase_deg of num_samples samples; either output may be NULL.  mem names all the pointers of the call. */
int pfb_trace_samples(pfb_trace_handle* h, const void* iq, uint64_t num_samples, float* mag, float* phase_deg,
                      uint32_t mem);
/* Host only: B = max(1, ceil(num_samples / max_bins)), the bin that shows num_samples samples in at most max_bins
 * columns.  PFB_ERR_BAD_ARG when max_bins == 0 or B > 2^31. */
int pfb_trace_choose_bin(uint64_t num_samples, uint32_t max_bins, uint32_t* bin_samples);
/* One whole .iq record: format, bit width and length from its header (checked as pfb_dwell_from_iq_file checks it),
 * B from pfb_trace_choose_bin, the payload streamed as pfb_stft_process_iq_file streams it; the final partial bin is
 * included.  `out` is host memory; *bins_out = ceil(numSamples / B), also on PFB_ERR_CAPACITY. */
int pfb_trace_envelope_from_iq_file(const char* path, uint32_t max_bins, pfb_trace_bin* out, uint64_t capacity_bins,
                                    uint64_t* bins_out, uint32_t* bin_samples_out, pfb_iq_info* info_out,
                                    int32_t device_id);

/* ---- matched filter (pulse compression) ---------------------------------------------------------------
 * Finds a coded pulse by its replica instead of its envelope.  The pulses are the reference's own:
 *   matlab/generate_pulsed_iq.m:17-19,43-59            LFM sweeps and Barker-13 chips (pfb_synth_* makes them)
 *   tx_rx_pulses_usrp.cpp:24,141-142,212-242,284-291   a 13-chip burst transmitted and the dwell received, written as
 *                                                      two .iq records, each with its own sampleStartTime
 *   matlab/generate_training_iq.m:16-22                pulse widths up to 1000 us: 56 000 samples at 56 MS/s
 * Arithmetic, with r[0..K-1] the caller's complex64 replica, 1 <= K <= 65536:
 *   x[n] = (I[n] + jQ[n]) / 2^(bit_width-1)            (cf32: as given)
 *   y[m] = g * sum_{n=0}^{K-1} conj(r[n]) * x[m+n]        m = 0, 1, ...  (stream-absolute)
 * g = 1; with PFB_MF_NORMALIZE g = 1/sum|r|^2 (float64, at create): a copy of r with amplitude A gives y = A at the
 * match.  Only complete windows are produced: N stream samples so far give max(0, N-K+1) outputs, and output m is the
 * index of the sample at which a pulse equal to the replica starts.  PFB_MF_COMPLEX stores y (complex64, 8 bytes per
 * output), PFB_MF_POWER |y|^2 (float32, 4 bytes).
 * Method: overlap-save fast convolution in fp32 with FFTs of fft_length points.  PFB_MF_ROUTE_FUSED (K <= fft_length/2)
 * is one kernel, fft_length - K + 1 outputs per block; PFB_MF_ROUTE_PARTITIONED (any K) cuts the replica into
 * ceil(K / (fft_length/2)) partitions, fft_length/2 outputs per block, through a device workspace the handle owns
 * (grow-only, at most 64 MiB, freed at destroy).  PFB_MF_ROUTE_AUTO: fused when K <= fft_length/2 (K <= 2048 for
 * fft_length = 0), partitioned above.  fft_length = 0 is the library's choice, the faster length per K range as
 * measured on the MI355X: fused, 1024 for K <= 64, 2048 for K <= 1024, 4096 above; partitioned,
 * 2048 for K <= 1024, 4096 above.
 * The handle is stateful like pfb_stft_*: it carries the last min(N, K-1) samples, so a stream may be cut into calls of
 * any length, length 0 included.  The same sequence of calls gives the same bits every time.  Different cuttings of one
 * stream agree to |y - y'| <= 2e-5 * g * ||r||_2 * max_m ||x[m..m+K-1]||_2 and are NOT bit-identical: the blocks start
 * where a call (or a staging step of a host-pointer call) starts.  A cf32 sample that is not finite may make every
 * output of the FFT block it falls in non-finite, not only the K outputs whose window holds it; it never causes a
 * fault or an access outside the buffers.
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers, a wrong
 * struct_size, K = 0, a replica value that is not finite, an all-zero replica with PFB_MF_NORMALIZE, a replica whose
 * scaled spectrum does not fit float32, an unknown output, flag or route, fft_length outside {0, 1024, 2048, 4096}, an
 * unknown mem, a device pointer not aligned to one sample (iq) or one output element (out).  PFB_ERR_BAD_FORMAT: an
 * unknown sample format, bit_width outside 1..8 (int8) or 1..16 (int16; ignored for cf32).  PFB_ERR_UNSUPPORTED:
 * K > 65536, or PFB_MF_ROUTE_FUSED with K > fft_length/2 (K > 2048 when fft_length = 0).  Then PFB_ERR_NO_DEVICE
 * without a HIP device. */
enum { PFB_MF_COMPLEX = 0, PFB_MF_POWER = 1 };
enum { PFB_MF_NORMALIZE = 1u << 0 };
enum { PFB_MF_ROUTE_AUTO = 0, PFB_MF_ROUTE_FUSED = 1, PFB_MF_ROUTE_PARTITIONED = 2 };

typedef struct pfb_mf_config {
  uint32_t struct_size;      /* = sizeof(pfb_mf_config)                                          */
  uint32_t replica_length;   /* K                                                                */
  const float* replica;      /* K interleaved re,im, finite, copied at create                    */
  uint32_t sample_format;    /* pfb_sample_format                                                */
  uint32_t bit_width;        /* full scale 2^(bit_width-1); ignored for CF32                     */
  uint32_t output;           /* PFB_MF_COMPLEX / PFB_MF_POWER                                    */
  uint32_t flags;            /* PFB_MF_NORMALIZE                                                 */
  uint32_t fft_length;       /* 0 = the library's choice, else 1024 / 2048 / 4096                */
  uint32_t route;            /* PFB_MF_ROUTE_*                                                   */
  int32_t device_id;         /* HIP device ordinal, -1 = current device                          */
} pfb_mf_config;

typedef struct pfb_mf_plan { /* what pfb_mf_describe reports; host only                          */
  uint32_t fft_length;       /* 1024 / 2048 / 4096                                               */
  uint32_t route;            /* PFB_MF_ROUTE_FUSED or PFB_MF_ROUTE_PARTITIONED                   */
  uint32_t partitions;       /* 1 (fused), ceil(K / (fft_length/2)) (partitioned)                */
  uint32_t block_outputs;    /* outputs per workgroup: fft_length - K + 1, or fft_length/2       */
  uint64_t workspace_bytes;  /* the most the handle's workspace grows to: 0 (fused), <= 64 MiB   */
} pfb_mf_plan;

typedef struct pfb_mf_handle pfb_mf_handle;

/* Host only: validate cfg (everything pfb_mf_create checks before the device) and report the plan. */
int pfb_mf_describe(const pfb_mf_config* cfg, pfb_mf_plan* plan_out);
/* Lifecycle as pfb_stft_*.  The handle owns the replica's spectra, the carried samples and the workspace. */
int pfb_mf_create(const pfb_mf_config* cfg, pfb_mf_handle** out);
int pfb_mf_destroy(pfb_mf_handle* h);
int pfb_mf_reset(pfb_mf_handle* h);   /* stream position back to 0, nothing carried */
int pfb_mf_set_stream(pfb_mf_handle* h, void* hip_stream);
int pfb_mf_sync(pfb_mf_handle* h);
int pfb_mf_get_device(const pfb_mf_handle* h, int* device_id);
/* The outputs the next call of num_samples samples completes. */
int pfb_mf_outputs_for(const pfb_mf_handle* h, uint64_t num_samples, uint64_t* outputs_out);
/* The stream index m of the next output to be produced: max(0, N-K+1) after N samples. */
int pfb_mf_next_index(const pfb_mf_handle* h, uint64_t* index_out);
/* Filter num_samples samples; the outputs they complete go to `out` (room for capacity_outputs), their number to
 * *outputs_out.  PFB_ERR_CAPACITY sets *outputs_out to the number needed and changes no state.  mem: iq and out are
 * both host pointers (PFB_MEM_HOST, staged as pfb_stft_process stages them, an output playing the role of a frame) or
 * both device pointers (PFB_MEM_DEVICE).  Synchronous. */
int pfb_mf_process(pfb_mf_handle* h, const void* iq, uint64_t num_samples, void* out, uint64_t capacity_outputs,
                   uint64_t* outputs_out, uint32_t mem);
/* Same, device pointers, enqueued on the handle's stream without a host sync (a partitioned call that grows the
 * workspace waits for the device). */
int pfb_mf_process_async(pfb_mf_handle* h, const void* d_iq, uint64_t num_samples, void* d_out,
                         uint64_t capacity_outputs, uint64_t* outputs_out);
/* One .iq record from disk (format and bit width checked against the handle), streamed as pfb_stft_process_iq_file
 * streams it; `out` is host memory.  The handle's state carries on from earlier calls: reset first for a record on
 * its own. */
int pfb_mf_process_iq_file(pfb_mf_handle* h, const char* path, void* out, uint64_t capacity_outputs,
                           uint64_t* outputs_out, pfb_iq_info* info_out);
/* Name of the kernel the last process call launched ("" before the first). */
const char* pfb_mf_last_kernel(const pfb_mf_handle* h);

/* ---- time-binned waterfalls of channelizer and STFT output ---------------------------------------------
 * Replaces the arithmetic of the reference's two-dimensional pictures (drawing stays with the caller):
 *   matlab/channelizer_example.m:56-71                  surf of abs(channelizer(x)), one window after another
 *   matlab/generate_channelized_training_iq.m:100-108   surf(f,t,abs(chan_iq))
 *   matlab/spectrogram_my_iq.m:114-115                  mesh of abs(s).^2
 * Input: a matrix of `rows` rows (frames) by W = width columns (channels, or STFT frequency rows), 1 <= W <= 65536.
 * Per element, by pfb_wf_config.element:
 *   PFB_WF_COMPLEX    complex64: p = (double)re*(double)re + (double)im*(double)im; the products are exact in double,
 *                     so contraction cannot change the result
 *   PFB_WF_MAGNITUDE  float32 a: p = (double)a*(double)a
 *   PFB_WF_POWER      float32 v: p = (double)v
 * Layout, ld in elements (a value smaller than the dense one is PFB_ERR_BAD_ARG):
 *   PFB_WF_ROWS       x[m*ld + k]: the channelizer's frame-major output and the STFT's out[m*nfft + r]; ld = 0 means W
 *   PFB_WF_COLUMNS    x[k*ld + m]: the channelizer's channel-major output; ld = 0 means this call's `rows`
 * Bins and cells: the rows are cut into bins of bin_rows = B consecutive rows (1 .. 2^24), counted from the handle's
 * origin (0 after create / reset; pfb_wf_flush starts a new grid at the next row).  Each completed bin gives W cells of
 * 16 bytes, bin-major: out[b*W + k] is bin b of column k.
 * Guarantees:
 *   - power_max, power_min and peak_row are exact selections (taken on the double p, the first row winning among equal
 *     powers): the same bits under any cutting of the rows into calls, either layout, any ld and any pointer alignment,
 *     and whether the matrix is in device memory, in host memory or made from a file by pfb_wf_from_*_iq_file.
 *   - power_mean is a double sum divided by the count, then rounded to float32.  The sum is taken without
 *     floating-point atomics in an order fixed by the call's lengths and its pointer's alignment to 16 bytes: the same
 *     call gives the same bits every time, another cutting may move the last bit.
 *   - Inputs must be finite: a non-finite element may leave the cells of its own (bin, column) unspecified; it never
 *     disturbs another cell, never faults and never causes an access outside the buffers.
 *   - No sqrt and no log10 run on the device: magnitude and dB are the host's, one value per cell.
 * Every argument is validated before the device is touched.  PFB_ERR_BAD_ARG: null pointers, a wrong struct_size, width
 * outside 1 .. 65536, bin_rows outside 1 .. 2^24, an unknown element, layout or mem, any flag bit (none is defined),
 * PFB_WF_COLUMNS with PFB_MEM_HOST, a device x not aligned to one element, out not aligned to 16 bytes.  Then
 * PFB_ERR_NO_DEVICE without a HIP device. */
enum { PFB_WF_COMPLEX = 0, PFB_WF_MAGNITUDE = 1, PFB_WF_POWER = 2 };
enum { PFB_WF_ROWS = 0, PFB_WF_COLUMNS = 1 };

typedef struct pfb_wf_cell {
  float power_max, power_mean, power_min;  /* (float) of the double value, round to nearest even                  */
  uint32_t peak_row;                       /* offset inside the bin (0 .. B-1) of the FIRST row holding the max   */
} pfb_wf_cell;

typedef struct pfb_wf_config {
  uint32_t struct_size;  /* = sizeof(pfb_wf_config)                 */
  uint32_t width;        /* W, 1 .. 65536                           */
  uint32_t bin_rows;     /* B, 1 .. 2^24                            */
  uint32_t element;      /* PFB_WF_COMPLEX / MAGNITUDE / POWER      */
  uint32_t layout;       /* PFB_WF_ROWS / PFB_WF_COLUMNS            */
  uint32_t flags;        /* 0                                       */
  int32_t device_id;     /* HIP device ordinal, -1 = current device */
} pfb_wf_config;

typedef struct pfb_wf_handle pfb_wf_handle;

/* Lifecycle as pfb_trace_*.  The handle holds the row position and, on the device, the bin a call left open. */
int pfb_wf_create(const pfb_wf_config* cfg, pfb_wf_handle** out);
int pfb_wf_destroy(pfb_wf_handle* h);
int pfb_wf_reset(pfb_wf_handle* h);   /* origin back to 0, no open bin */
int pfb_wf_set_stream(pfb_wf_handle* h, void* hip_stream);
int pfb_wf_sync(pfb_wf_handle* h);
int pfb_wf_get_device(const pfb_wf_handle* h, int* device_id);
/* The bins the next call of `rows` rows completes. */
int pfb_wf_bins_for(const pfb_wf_handle* h, uint64_t rows, uint64_t* bins_out);
/* The cells of the bins these rows complete, to `out` (room for capacity_bins * W cells); *bins_out = their number.
 * PFB_ERR_CAPACITY sets *bins_out to the number needed and changes no state.  mem: x and out are both device pointers
 * (PFB_MEM_DEVICE) or both host pointers (PFB_MEM_HOST, PFB_WF_ROWS only, staged as pfb_stft_process stages them: a row
 * playing the role of a sample, a bin of W cells that of a frame, steps of at most 64 MiB per side).  Synchronous. */
int pfb_wf_process(pfb_wf_handle* h, const void* x, uint64_t rows, uint64_t ld, pfb_wf_cell* out,
                   uint64_t capacity_bins, uint64_t* bins_out, uint32_t mem);
/* Same, device pointers, enqueued on the handle's stream without a host sync (bins longer than the row tile use a
 * device scratch that grows with the longest call so far: a call that grows it waits for the device). */
int pfb_wf_process_async(pfb_wf_handle* h, const void* d_x, uint64_t rows, uint64_t ld, pfb_wf_cell* d_out,
                         uint64_t capacity_bins, uint64_t* bins_out);
/* The open bin's W cells to host memory (*rows_in_bin = the rows it holds, 0 when none is open: nothing is written);
 * the mean is over the rows present.  A new bin grid starts at the next row. */
int pfb_wf_flush(pfb_wf_handle* h, pfb_wf_cell* out_host, uint32_t* rows_in_bin);
/* Host only: B = max(1, ceil(rows / max_bins)), the bin that shows `rows` rows in at most max_bins image rows.
 * PFB_ERR_BAD_ARG when max_bins == 0 or B > 2^24. */
int pfb_wf_choose_bin(uint64_t rows, uint32_t max_bins, uint32_t* bin_rows);
/* One whole .iq record to an image without its channel matrix ever existing in full: the header is checked as in
 * pfb_process_iq_file, the handle is reset, B = pfb_wf_choose_bin(the frames the record gives, max_bins), and the
 * payload is streamed in chunks of chunk_samples samples (0 = 2^24): each is copied in, transformed by
 * pfb_process_async into a device scratch sized for one chunk and reduced from there, all on the handle's stream.  The
 * final partial bin is included.  Element kind and layout follow the handle (complex, PFB_FLAG_MAGNITUDE, + PFB_FLAG_POWER;
 * frame-major or channel-major).  `out` is host memory with room for capacity_bins * M cells; *bins_out =
 * ceil(frames / B), also on PFB_ERR_CAPACITY; *bin_rows_out = B. */
int pfb_wf_from_channelizer_iq_file(pfb_handle* ch, const char* path, uint32_t max_bins, uint64_t chunk_samples,
                                    pfb_wf_cell* out, uint64_t capacity_bins, uint64_t* bins_out,
                                    uint32_t* bin_rows_out, pfb_iq_info* info_out);
/* The same loop over pfb_stft_process_async: W = nfft, PFB_STFT_COMPLEX gives PFB_WF_COMPLEX and PFB_STFT_POWER gives
 * PFB_WF_POWER; a PFB_STFT_DB handle is PFB_ERR_BAD_ARG (averaging dB is not averaging power). */
int pfb_wf_from_stft_iq_file(pfb_stft_handle* st, const char* path, uint32_t max_bins, uint64_t chunk_samples,
                             pfb_wf_cell* out, uint64_t capacity_bins, uint64_t* bins_out, uint32_t* bin_rows_out,
                             pfb_iq_info* info_out);

/* ---- channel synthesizer: an I/Q stream rebuilt from channelizer output ---------------------------------
 * The twin of pfb_process: it reads exactly what a frame-major channelizer handle writes and puts the channels back
 * together at the full rate, all of them or the ones a weight mask keeps (the emitter pfb_pdw_from_iq_file reported in
 * column `bin`, alone, as a time signal for pfb_mf_*, pfb_dwell_analyze or pfb_trace_*).
 * Input: frame m = 0, 1, ... (stream-absolute) is M complex64 values at y[m*ld + c], ld >= M (ld = 0 means M).
 * Column c holds channel k = c, or, with PFB_CHSYN_FFTSHIFT, k = (c + ceil(M/2)) mod M: the columns a handle made
 * with PFB_FLAG_FFTSHIFT writes.  Per frame, with w an optional real float32 weight per COLUMN (NULL = all ones; a 0/1
 * mask isolates a band):
 *   v_m[p] = sum_k w[c(k)] * y[m, c(k)] * e^{+j 2 pi k p / M}          p = 0 .. M-1
 * Per output sample s = b*D + d, 0 <= d < D, with g[0 .. L_g-1] the synthesis taps, L_g = M*P_g and Q = L_g / D:
 *   x[s] = scale * sum_{q=0}^{Q-1} g[d + q*D] * v_{b-q}[(d + q*D) mod M]
 * Frames before frame 0 are zero; the sum is always taken in ascending q.  With PFB_CHSYN_DEROTATE the input was made
 * under PFB_FLAG_DEROTATE: v_m is then read at (p + m*D) mod M, an index change (the identity for D = M), which is why
 * the handle keeps the absolute frame index (pfb_chsyn_set_frame_index for a stream that starts elsewhere).
 * F frames in give exactly F*D samples out; a call of 0 frames is legal; feeding Q-1 zero frames drains the tail.
 * scale = 0 means D, the unity-gain value when the analysis and the synthesis taps both have DC gain 1.
 * Output: PFB_FMT_CF32, interleaved float I,Q, or PFB_FMT_INT16_IQ, round(x * 2^(bit_width-1)) with halves away from
 * zero, saturated to -2^(bit_width-1) .. 2^(bit_width-1)-1 (a NaN stores 0) -- a result that can be written back as a
 * record with pfb_iq_serialize_header.
 * Reconstruction.  A channelizer with taps h (length L_h) and this synthesizer with taps g return the input delayed by
 *   delta = L_h/2 + L_g/2 - input_offset   samples
 * to the accuracy the pair of filters allows.  For the 2x oversampled bank, D = M/2, with h =
 * pfb_design_prototype(M, 12) and g = pfb_design_prototype(D, 24) (length 12*M), the error is 3.6e-5 of the signal
 * (-89 dB) and the gain 1.0000001 (float64, M = 16, 56, 64).  For the critically sampled bank, D = M, with g = h the
 * Kaiser-windowed sinc is a Nyquist filter and not a root-Nyquist one: the sum above is computed all the same, but it
 * reconstructs only to about 20 %.  Reconstruction quality at D = M is the business of the caller's taps.
 * Domain: 2 <= M <= 4096; D = M (decimation = 0 or M) or D = M/2 for even M; 1 <= P_g <= 24; the taps finite float32,
 * copied at create.  Channel-major input (pfb_chsyn_config.layout = PFB_LAYOUT_CHANNEL_MAJOR) is PFB_ERR_UNSUPPORTED.
 * Method: packed fp32.  PFB_CHSYN_ROUTE_GENERIC (any M) is two launches: the M-point DFTs of a chunk of frames into a
 * device workspace the handle owns (grow-only, at most 64 MiB, freed at destroy), then the Q-term sums out of it.
 * PFB_CHSYN_ROUTE_FUSED (M = 56, 64, 128, 256, both D, both outputs, as long as tile_frames + Q - 1 rows fit 64 KiB of
 * LDS) is one launch: a workgroup owns tile_frames consecutive output blocks and keeps the rows they need in LDS.
 * PFB_CHSYN_ROUTE_AUTO takes the fused route where there is one.  The handle carries the last Q-1 rows v_m in device
 * memory.  A frame's v_m does not depend on where the frame sits in a tile, a call, a chunk or a staging step, so
 * within one route the output is THE SAME BITS under any cutting of the frame stream into calls.  The two routes
 * differ by rounding only.
 * Elements that are not finite poison only the Q*D output samples their frame reaches; they never cause a fault or an
 * access outside the buffers.
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers, a wrong
 * struct_size, M < 2, P_g = 0, a decimation other than 0, M or M/2 (M even), a tap or a scale that is not finite, an
 * unknown flag, route or layout, an unknown mem, ld < M, a device pointer not aligned to 8 bytes (y) or to one output
 * sample (out).  PFB_ERR_BAD_FORMAT: an output format other than PFB_FMT_CF32 / PFB_FMT_INT16_IQ, bit_width outside
 * 2..16 (int16; ignored for cf32).  PFB_ERR_UNSUPPORTED: M > 4096, P_g > 24 (the taps of such a shape are not looked
 * at), channel-major input, PFB_CHSYN_ROUTE_FUSED for a shape without a fused kernel.  Then PFB_ERR_NO_DEVICE without a
 * HIP device. */
enum { PFB_CHSYN_FFTSHIFT = 1u << 0, PFB_CHSYN_DEROTATE = 1u << 1 };
enum { PFB_CHSYN_ROUTE_AUTO = 0, PFB_CHSYN_ROUTE_FUSED = 1, PFB_CHSYN_ROUTE_GENERIC = 2 };

typedef struct pfb_chsyn_config {
  uint32_t struct_size;       /* = sizeof(pfb_chsyn_config)                                       */
  uint32_t num_channels;      /* M                                                                */
  uint32_t taps_per_channel;  /* P_g: the synthesis taps have M*P_g values                        */
  uint32_t decimation;        /* D: 0 or M = critically sampled, M/2 = 2x oversampled             */
  const float* taps;          /* g[0 .. M*P_g-1], finite, copied at create                        */
  double scale;               /* 0 = D                                                            */
  uint32_t output_format;     /* PFB_FMT_CF32 / PFB_FMT_INT16_IQ                                  */
  uint32_t bit_width;         /* int16 output: full scale 2^(bit_width-1), 2..16                  */
  uint32_t layout;            /* pfb_output_layout of the INPUT; PFB_LAYOUT_FRAME_MAJOR only      */
  uint32_t flags;             /* PFB_CHSYN_*                                                      */
  uint32_t route;             /* PFB_CHSYN_ROUTE_*                                                */
  int32_t device_id;          /* HIP device ordinal, -1 = current device                          */
} pfb_chsyn_config;

typedef struct pfb_chsyn_plan { /* what pfb_chsyn_describe reports; host only                     */
  uint32_t route;             /* PFB_CHSYN_ROUTE_FUSED or PFB_CHSYN_ROUTE_GENERIC                 */
  uint32_t decimation;        /* D                                                                */
  uint32_t q;                 /* Q = M*P_g / D: the frames one output sample sums over            */
  uint32_t tile_frames;       /* output blocks per workgroup (fused), frames per DFT tile (generic) */
  uint64_t carried_bytes;     /* the Q-1 carried rows: (Q-1)*M*8                                  */
  uint64_t workspace_bytes;   /* the most the workspace grows to: 0 (fused), <= 64 MiB            */
} pfb_chsyn_plan;

typedef struct pfb_chsyn_handle pfb_chsyn_handle;

/* Host only: validate cfg (everything pfb_chsyn_create checks before the device) and report the plan. */
int pfb_chsyn_describe(const pfb_chsyn_config* cfg, pfb_chsyn_plan* plan_out);
/* Lifecycle as pfb_mf_*.  The handle owns the taps, the weights, the carried rows and the workspace. */
int pfb_chsyn_create(const pfb_chsyn_config* cfg, pfb_chsyn_handle** out);
int pfb_chsyn_destroy(pfb_chsyn_handle* h);
int pfb_chsyn_reset(pfb_chsyn_handle* h);   /* nothing carried, frame index 0; the weights stay */
int pfb_chsyn_set_stream(pfb_chsyn_handle* h, void* hip_stream);
int pfb_chsyn_sync(pfb_chsyn_handle* h);
int pfb_chsyn_get_device(const pfb_chsyn_handle* h, int* device_id);
/* Absolute index m of the next frame (what PFB_CHSYN_DEROTATE reads its rows by); the carried rows stay and are the
 * frames next_frame-1, next_frame-2, ... from then on. */
int pfb_chsyn_set_frame_index(pfb_chsyn_handle* h, uint64_t next_frame);
int pfb_chsyn_get_frame_index(const pfb_chsyn_handle* h, uint64_t* next_frame);
/* The samples a call of num_frames frames writes: num_frames * D. */
int pfb_chsyn_samples_for(const pfb_chsyn_handle* h, uint64_t num_frames, uint64_t* samples_out);
/* M weights from host memory (NULL: all ones), in effect from the next frame on: frames already taken keep theirs.
 * Waits for what the handle's stream has queued. */
int pfb_chsyn_set_weights(pfb_chsyn_handle* h, const float* weights);
/* Synthesize num_frames frames; their num_frames*D samples go to `out` (room for capacity_samples), their number to
 * *samples_out.  PFB_ERR_CAPACITY sets *samples_out to the number needed and changes no state.  mem: y and out are
 * both host pointers (PFB_MEM_HOST, staged as pfb_stft_process stages them, a frame of ld values playing the role of
 * a sample and D output samples that of a frame, steps of at most 64 MiB per side) or both device pointers
 * (PFB_MEM_DEVICE).  Synchronous. */
int pfb_chsyn_process(pfb_chsyn_handle* h, const void* y, uint64_t num_frames, uint64_t ld, void* out,
                      uint64_t capacity_samples, uint64_t* samples_out, uint32_t mem);
/* Same, device pointers, enqueued on the handle's stream without a host sync (a generic call that grows the workspace
 * waits for the device). */
int pfb_chsyn_process_async(pfb_chsyn_handle* h, const void* d_y, uint64_t num_frames, uint64_t ld, void* d_out,
                            uint64_t capacity_samples, uint64_t* samples_out);
/* Name of the kernel the last process call launched ("" before the first). */
const char* pfb_chsyn_last_kernel(const pfb_chsyn_handle* h);

/* ---- matched-filter bank: delay and carrier of a coded pulse ---------------------------------------------
 * pfb_mf_* finds a pulse only at the carrier its replica was made for, and the reference's signals do not give one:
 *   matlab/generate_pulsed_iq.m:13, generate_training_iq.m:13   the carrier is drawn at random in +-fs/2
 *   tx_rx_pulses_usrp.cpp                                       the TX / RX pair comes from two oscillators
 * A Barker-13 pulse of 13 x 39 samples keeps 0.41 of its peak power one bin of a 1024-point FFT off its carrier and
 * 0.0066, at a wrong sample, 37 bins off.  The bank correlates with H replicas, each the caller's modulated to one
 * frequency offset, and shares the load and the forward FFT of a block among them.
 * Arithmetic, with x, r, K and g as the matched filter defines them (g by PFB_MF_NORMALIZE in pfb_mfbank_config.flags):
 *   q_h    = (first_bin + h) * bin_step                    h = 0 .. H-1, first_bin may be negative
 *   f_h    = q_h * fs / fft_length                         the offset hypothesis h assumes (pfb_mfbank_frequencies)
 *   y_h[m] = g * sum_{n=0}^{K-1} conj(r[n]) * e^{-j 2 pi q_h n / fft_length} * x[m+n]
 *   p_h[m] = |y_h[m]|^2
 * The modulation is anchored at the replica's first sample: y_h[m] does not depend on where a block or a call starts.
 * Outputs are stream-absolute and only complete windows are produced: N samples so far give max(0, N-K+1) outputs,
 * exactly as pfb_mf_*.  Steps of whole bins are enough: a pulse of K <= fft_length/2 samples that lies half a bin from
 * the nearest hypothesis keeps sinc(K / (2 fft_length)) of its amplitude there, 0.900 (-0.91 dB) at K = fft_length/2
 * and more for every shorter replica.
 * Outputs, by pfb_mfbank_config.output:
 *   PFB_MFBANK_BEST     one pfb_mfbank_cell per output m: the largest p_h[m] over h and the h that gave it.  The
 *                       selection starts from h = 0 and replaces only on a strictly greater power: ties go to the
 *                       lowest h and a power that is not a number never displaces anything (p_0[m] = NaN stays, h = 0).
 *   PFB_MFBANK_SURFACE  float32 p_h[m] at out[h * row_pitch + m], the ambiguity picture; row_pitch, in elements, is
 *                       given per call and must be >= the outputs the call completes; `out` holds
 *                       (H-1) * row_pitch + outputs elements.  PFB_MFBANK_BEST ignores row_pitch.
 * Method: pfb_mf_*'s fused route only, 1 <= K <= fft_length/2, fft_length 1024, 2048 or 4096; fft_length = 0 means
 * 4096, so that the bins of first_bin and bin_step do not depend on K.  One workgroup per block of fft_length - K + 1
 * outputs transforms the block once and runs the inverse transform H times on a rotated read of the one spectrum table.
 * State, cutting and rounding as pfb_mf_*: the last min(N, K-1) samples are carried, the same sequence of calls gives the
 * same bits, different cuttings agree to pfb_mf_*'s tolerance per hypothesis (blocks start where a call or a staging
 * step starts); a sample that is not finite may spoil every output of the FFT blocks it falls in and nothing else.
 * Every argument is validated before the device is touched, in pfb_mf_create's order and with its codes.
 * PFB_ERR_BAD_ARG: null pointers, a wrong struct_size, K = 0, an unknown output or flag, fft_length outside {0, 1024,
 * 2048, 4096}, bin_step = 0, H = 0, H * bin_step > fft_length (two hypotheses would coincide); then a replica value
 * that is not finite, an all-zero replica with PFB_MF_NORMALIZE; an unknown mem, row_pitch below the call's outputs
 * (surface), a device pointer not aligned to one sample (iq) or one output element (out: 8 bytes best, 4 surface).
 * PFB_ERR_BAD_FORMAT: an unknown sample format, bit_width outside 1..8 (int8) or 1..16 (int16; ignored for cf32).
 * PFB_ERR_UNSUPPORTED: K > fft_length/2, the code pfb_mf_create gives for PFB_MF_ROUTE_FUSED with such a replica.  Then
 * PFB_ERR_BAD_ARG for a replica whose scaled spectrum does not fit float32, and PFB_ERR_NO_DEVICE without a HIP device,
 * last. */
enum { PFB_MFBANK_BEST = 0, PFB_MFBANK_SURFACE = 1 };

typedef struct pfb_mfbank_config {
  uint32_t struct_size;      /* = sizeof(pfb_mfbank_config)                                      */
  uint32_t replica_length;   /* K                                                                */
  const float* replica;      /* K interleaved re,im, finite, copied at create                    */
  uint32_t sample_format;    /* pfb_sample_format                                                */
  uint32_t bit_width;        /* full scale 2^(bit_width-1); ignored for CF32                     */
  uint32_t output;           /* PFB_MFBANK_BEST / PFB_MFBANK_SURFACE                             */
  uint32_t flags;            /* PFB_MF_NORMALIZE                                                 */
  uint32_t fft_length;       /* 0 = 4096, else 1024 / 2048 / 4096                                */
  int32_t first_bin;         /* q_0 = first_bin * bin_step                                       */
  uint32_t num_hypotheses;   /* H >= 1, H * bin_step <= fft_length                               */
  uint32_t bin_step;         /* >= 1                                                             */
  int32_t device_id;         /* HIP device ordinal, -1 = current device                          */
} pfb_mfbank_config;

typedef struct pfb_mfbank_plan { /* what pfb_mfbank_describe reports; host only                  */
  uint32_t fft_length;       /* 1024 / 2048 / 4096                                               */
  uint32_t block_outputs;    /* outputs per workgroup: fft_length - K + 1                        */
  uint32_t num_hypotheses;   /* H                                                                */
  uint32_t lds_bytes;        /* LDS of one workgroup: two fft_length-point complex buffers       */
} pfb_mfbank_plan;

typedef struct pfb_mfbank_cell { /* one output of PFB_MFBANK_BEST                                */
  float power;               /* max over h of p_h[m]                                             */
  int32_t hypothesis;        /* the h that gave it                                               */
} pfb_mfbank_cell;

typedef struct pfb_mfbank_handle pfb_mfbank_handle;

/* Host only: validate cfg (everything pfb_mfbank_create checks before the device) and report the plan. */
int pfb_mfbank_describe(const pfb_mfbank_config* cfg, pfb_mfbank_plan* plan_out);
/* Host only: out[h] = f_h = (first_bin + h) * bin_step * fs / fft_length for h = 0 .. H-1 (not wrapped into +-fs/2).
 * Reads struct_size, fft_length, first_bin, num_hypotheses and bin_step of cfg and nothing else: the replica may be
 * NULL.  PFB_ERR_BAD_ARG for null pointers, a wrong struct_size, a grid pfb_mfbank_create refuses or fs not finite. */
int pfb_mfbank_frequencies(const pfb_mfbank_config* cfg, double fs, double* out);
/* Lifecycle, stream, sync, device, outputs_for, next_index and last_kernel as pfb_mf_*. */
int pfb_mfbank_create(const pfb_mfbank_config* cfg, pfb_mfbank_handle** out);
int pfb_mfbank_destroy(pfb_mfbank_handle* h);
int pfb_mfbank_reset(pfb_mfbank_handle* h);   /* stream position back to 0, nothing carried */
int pfb_mfbank_set_stream(pfb_mfbank_handle* h, void* hip_stream);
int pfb_mfbank_sync(pfb_mfbank_handle* h);
int pfb_mfbank_get_device(const pfb_mfbank_handle* h, int* device_id);
int pfb_mfbank_outputs_for(const pfb_mfbank_handle* h, uint64_t num_samples, uint64_t* outputs_out);
int pfb_mfbank_next_index(const pfb_mfbank_handle* h, uint64_t* index_out);
/* Process num_samples samples; the outputs they complete go to `out`, their number to *outputs_out.  capacity_outputs
 * counts outputs: cells (best), elements of one row (surface).  PFB_ERR_CAPACITY sets *outputs_out to the number
 * needed and changes no state.  mem: iq and out are both host pointers (PFB_MEM_HOST, staged as pfb_mf_process stages
 * them; a surface walks in steps whose H rows fit the 64 MiB staging, 2^24 / H outputs each) or both device pointers
 * (PFB_MEM_DEVICE).  Synchronous. */
int pfb_mfbank_process(pfb_mfbank_handle* h, const void* iq, uint64_t num_samples, void* out, uint64_t capacity_outputs,
                       uint64_t row_pitch, uint64_t* outputs_out, uint32_t mem);
/* Same, device pointers, enqueued on the handle's stream without a host sync. */
int pfb_mfbank_process_async(pfb_mfbank_handle* h, const void* d_iq, uint64_t num_samples, void* d_out,
                             uint64_t capacity_outputs, uint64_t row_pitch, uint64_t* outputs_out);
/* One .iq record from disk (format and bit width checked against the handle), streamed as pfb_mf_process_iq_file
 * streams it; `out` is host memory.  The handle's state carries on from earlier calls: reset first for a record on
 * its own. */
int pfb_mfbank_process_iq_file(pfb_mfbank_handle* h, const char* path, void* out, uint64_t capacity_outputs,
                               uint64_t row_pitch, uint64_t* outputs_out, pfb_iq_info* info_out);
/* Name of the kernel the last process call launched ("" before the first). */
const char* pfb_mfbank_last_kernel(const pfb_mfbank_handle* h);


/* ---- CFAR detector: pulse lists from a compressed stream --------------------------------------
 * The matched filter and its bank leave a stream of powers on the device; this unit turns it into one record per
 * pulse.  A constant-false-alarm-rate detector estimates the noise around each cell from training cells on both sides,
 * scales it by a factor chosen for a false-alarm probability, joins the crossings into runs and reports each run's peak.
 * This comment is the definition: the device code (csrc/pfb_cfar.hip) and the tests' restatement (tests/cfar_ref.py)
 * are each written from it.
 *
 * Input: cells with the global index i = 0, 1, ... since create or reset, of one of two kinds
 *   PFB_CFAR_POWER      float32 p[i], what PFB_MF_POWER writes; hyp[i] = -1
 *   PFB_CFAR_BANK_CELL  pfb_mfbank_cell, what PFB_MFBANK_BEST writes: p[i] = cell.power, hyp[i] = cell.hypothesis
 * Parameters: block length C (a power of two, 4 .. 1024), guard blocks G (0 .. 64), training blocks per side T
 * (1 .. 32), method (CA, GO, SO), factor alpha (float32, finite, > 0), min_power (float32, >= 0), merge_gap g
 * (0 .. 2^20 cells).
 *
 * Blocks are aligned to the global index: block b holds cells bC .. bC+C-1.  That alignment makes every figure below
 * independent of how the stream is cut into calls.
 *
 * Block sum S[b], float32: the balanced binary tree over the block's C cells in index order -- level 0 adds cells 2j
 * and 2j+1, level 1 adds those sums pairwise, and so on; every node is one float32 addition.  (A lane's
 * (a0+a1)+(a2+a3) followed by xor-butterfly shuffles 1, 2, 4, ... is this sum: float addition is commutative, so
 * butterfly and tree agree bit for bit, and with additions only no FMA can arise.)  A block takes part in training
 * only when all its C cells exist ("complete").
 *
 * Noise of block b: the lead set is the blocks b-G-T .. b-G-1 that are >= 0 (nL of them), the lag set the blocks
 * b+G+1 .. b+G+T that are complete (nR).  sumL and sumR are float64 sums of the float32 S[.], sequential in ascending
 * block index.
 *   CA  noise = (float)((sumL + sumR) / ((nL + nR) * C))
 *   GO  noise = (float)max(sumL / (nL * C), sumR / (nR * C))       SO: the same with min
 * In GO and SO an empty side is left out, and a NaN on either side gives NaN.  All divisions are float64, with one
 * rounding to float32 at the end.  With both sets empty the block has no noise: none of its cells is ever over, and
 * they are counted in pfb_cfar_stats.cells_without_noise.
 *
 * Decision: over[i] = (p[i] > alpha * noise) && (p[i] > min_power), the product one float32 multiply.  A NaN on either
 * side of a comparison therefore never detects; an Inf cell is over (against a finite threshold) and blinds the blocks
 * that train on it.  That is IEEE behaviour, nothing is special-cased.
 *
 * When a block is decided: while streaming, block b is decided once block b+G+T is complete (blocks near the stream
 * start have a short or empty lead set).  pfb_cfar_flush ends the stream: every remaining block, a final partial one
 * included, is decided with the complete training blocks that exist; after it the handle takes cells only after
 * pfb_cfar_reset (PFB_ERR_BAD_ARG before).  Block b's decision depends only on the number of complete blocks at that
 * time, so without a flush it is a function of the total cell count alone.
 *
 * Detections: over cells whose gaps are <= g cells of not-over form one run.  A run whose last over cell is e closes
 * when g+1 decided cells follow e, or at flush.  A closed run yields one pfb_cfar_det, in ascending first_index.
 *
 * Invariance: the detections of any cutting of the stream into calls, concatenated and followed by flush, are the
 * same bytes as those of one call and flush.  Every figure is a fixed-order function of global indices: no float
 * atomics, no arrival-order sums, no running sums.
 *
 * Limits: training by whole blocks is a deliberate trade for that invariance and for side data of 1/C of the stream;
 * the guards must cover the replica's range sidelobes (G * C >= K) whatever the granularity.  C = 1 and 2 (the
 * cell-sliding window), OS-CFAR and a detector fused into the matched filter's store are not built.
 *
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers, a wrong
 * struct_size, an unknown element or method, a block_cells that is no power of two in 4 .. 1024, guard_blocks > 64,
 * train_blocks outside 1 .. 32, merge_gap > 2^20, an alpha that is not finite or <= 0, a min_power that is negative or
 * NaN, flags != 0.  Then PFB_ERR_NO_DEVICE without a HIP device. */
enum { PFB_CFAR_POWER = 0, PFB_CFAR_BANK_CELL = 1 };
enum { PFB_CFAR_CA = 0, PFB_CFAR_GO = 1, PFB_CFAR_SO = 2 };
#define PFB_CFAR_DET_ONE_SIDED 1u /* pfb_cfar_det.flags: the peak's block trained on fewer than 2T blocks */

typedef struct pfb_cfar_config {
  uint32_t struct_size;   /* = sizeof(pfb_cfar_config)                                        */
  uint32_t element;       /* PFB_CFAR_POWER / PFB_CFAR_BANK_CELL                              */
  uint32_t method;        /* PFB_CFAR_CA / GO / SO                                            */
  uint32_t block_cells;   /* C                                                                */
  uint32_t guard_blocks;  /* G                                                                */
  uint32_t train_blocks;  /* T, per side                                                      */
  uint32_t merge_gap;     /* g, cells                                                         */
  float alpha;
  float min_power;
  uint32_t flags;         /* 0                                                                */
  int32_t device_id;      /* -1 = the current device                                          */
} pfb_cfar_config;

typedef struct pfb_cfar_plan { /* what pfb_cfar_describe reports; host only                    */
  uint64_t latency_cells;  /* (G+T+1) * C: the most a cell waits for its decision              */
  uint64_t training_cells; /* 2 * T * C                                                        */
  uint64_t carry_bytes;    /* device bytes that hold the undecided cells and their block sums  */
  char sum_kernel[32];     /* the sum pass's tier for this C                                   */
} pfb_cfar_plan;

typedef struct pfb_cfar_det {        /* 48 bytes */
  uint64_t first_index, last_index;  /* first and last over cell of the run                                   */
  uint64_t peak_index;               /* the over cell of largest p, ties to the lowest index                  */
  float peak_power, noise;           /* p there; the noise of that cell's block                               */
  int32_t hypothesis;                /* hyp[peak_index]; -1 for PFB_CFAR_POWER                                */
  uint32_t cells_over;               /* over cells in the run, saturating at 2^32-1                           */
  uint32_t flags;                    /* PFB_CFAR_DET_ONE_SIDED: the peak's block trained on fewer than 2T blocks */
  uint32_t reserved;                 /* 0 */
} pfb_cfar_det;

typedef struct pfb_cfar_stats {
  uint64_t cells_in;            /* cells taken since create or reset                                          */
  uint64_t cells_decided;
  uint64_t cells_over;
  uint64_t cells_without_noise; /* decided cells of blocks with both training sets empty                      */
  uint64_t detections;          /* runs closed, the dropped ones included                                     */
  uint64_t dropped;             /* closed runs pfb_cfar_process_async had no room to write                    */
  uint64_t open_run;            /* 0 or 1: a run waits for its g+1 decided cells                              */
} pfb_cfar_stats;

typedef struct pfb_cfar_handle pfb_cfar_handle;

/* Host only: validate cfg (everything pfb_cfar_create checks before the device) and report the plan. */
int pfb_cfar_describe(const pfb_cfar_config* cfg, pfb_cfar_plan* plan_out);
/* Host only, float64: *alpha_out = N * (pfa^(-1/N) - 1), N = training_cells: the factor of CA-CFAR for square-law
 * detected (exponentially distributed) noise.  GO and SO have other factors; a caller that uses them passes its own
 * alpha.  PFB_ERR_BAD_ARG unless 0 < pfa < 1, N >= 1 and alpha_out is not null. */
int pfb_cfar_alpha(double pfa, uint64_t training_cells, double* alpha_out);
int pfb_cfar_create(const pfb_cfar_config* cfg, pfb_cfar_handle** out);
int pfb_cfar_destroy(pfb_cfar_handle* h);
int pfb_cfar_reset(pfb_cfar_handle* h);   /* stream index back to 0, nothing carried, stats zeroed */
int pfb_cfar_set_stream(pfb_cfar_handle* h, void* hip_stream);
int pfb_cfar_sync(pfb_cfar_handle* h);
int pfb_cfar_get_device(const pfb_cfar_handle* h, int* device_id);
int pfb_cfar_next_index(const pfb_cfar_handle* h, uint64_t* index_out);  /* global index of the next cell taken */
/* Synchronises the handle's stream: the device keeps the counts that depend on the data. */
int pfb_cfar_get_stats(pfb_cfar_handle* h, pfb_cfar_stats* stats_out);
/* Take num_cells cells and write the detections that close, in order, to det_out (room for `capacity`); their number
 * goes to *count_out.  PFB_ERR_CAPACITY sets *count_out to the number needed and changes no state (what det_out holds
 * is then unspecified).  mem: cells and det_out are both host pointers (PFB_MEM_HOST, the cells staged in steps of
 * 2^24) or both device pointers (PFB_MEM_DEVICE, cells aligned to one element, det_out to 8 bytes).  Synchronous. */
int pfb_cfar_process(pfb_cfar_handle* h, const void* cells, uint64_t num_cells, pfb_cfar_det* det_out, uint64_t capacity,
                     uint64_t* count_out, uint32_t mem);
/* End the stream: decide what is left and close the open run.  Capacity contract and mem (of det_out) as above. */
int pfb_cfar_flush(pfb_cfar_handle* h, pfb_cfar_det* det_out, uint64_t capacity, uint64_t* count_out, uint32_t mem);
/* Device pointers, enqueued on the handle's stream without a host sync.  *d_count_out (a uint64 in device memory) is
 * the number of runs the call closed.  Records beyond `capacity` are not written: they are counted in
 * pfb_cfar_stats.dropped, and the state advances. */
int pfb_cfar_process_async(pfb_cfar_handle* h, const void* d_cells, uint64_t num_cells, pfb_cfar_det* d_det_out,
                           uint64_t capacity, uint64_t* d_count_out);
/* Host only: detections as pulse descriptor words, so that pfb_event_fit takes them as it takes PDWs.
 *   toa = (peak_index + 1) / fs + sample_start_time (the extractors' 1-based convention)
 *   pw = (last_index - first_index + 1) / fs      snr = 10 log10(peak_power / noise)      mag = sqrt(peak_power)
 *   freq = fc + (first_bin + hypothesis) * bin_step * bin_hz when hypothesis >= 0 (bank input), fc otherwise
 *   sat = 0, bin = hypothesis
 * PFB_ERR_BAD_ARG for null pointers (with n > 0) or an fs that is not finite and > 0. */
int pfb_cfar_to_pdw(const pfb_cfar_det* dets, uint64_t n, double fs, double fc, double sample_start_time, double bin_hz,
                    int32_t first_bin, uint32_t bin_step, pfb_pdw* pdw_out);
/* Name of the sum kernel the last call launched ("" before the first). */
const char* pfb_cfar_last_kernel(const pfb_cfar_handle* h);

/* ---- pulse-Doppler integration: range-Doppler maps of a pulse train ---------------------------
 * Every unit above decides on one pulse at a time, yet the reference's signals are trains of identical pulses
 * (matlab/generate_pulsed_iq.m and generate_training_iq.m emit a pulse of PW every PRI, tx_rx_pulses_usrp.cpp:71 takes
 * the PRI as an argument, the training records carry PW and PRI in their names).  K compressed pulses folded at the PRI
 * add coherently, 10 log10 K dB over one pulse, and a phase step from pulse to pulse -- a carrier offset far finer than
 * one bin of the bank -- shows as a Doppler bin.  This comment is the definition: the device code (csrc/pfb_pd.hip)
 * and the tests' restatement (tests/pd_ref.py) are each written from it.
 *
 * Input: a complex64 stream x[n], n the stream-absolute index since create, reset or pfb_pd_set_index: what
 * PFB_MF_COMPLEX writes, or any cf32 stream.
 * Parameters: pri L samples (1 .. 2^24), origin o (the stream index of gate 0 of pulse 0, <= 2^62), num_gates R
 * (1 .. L), num_pulses K per coherent interval (CPI), doppler_length ND in {8, 16, 32, 64, 128, 256, 512, 1024}
 * (0: the smallest of these >= K), 1 <= K <= ND, a float32 window w[K] (NULL: all ones; finite, copied at create).
 *
 *   A_c[k][r] = x[o + (c K + k) L + r]       CPI c = 0, 1, ..., pulse k = 0 .. K-1, gate r = 0 .. R-1
 * CPIs do not overlap; samples before o and between the gates are ignored.  Rows K .. ND-1 of the transform are zero.
 * Outputs, by pfb_pd_config.output; c' counts the CPIs the call completes:
 *   PFB_PD_COMPLEX      Z_c[d][r] = sum_{k<K} w[k] A_c[k][r] e^{-j 2 pi d k / ND}, complex64 at out[(c' ND + d) R + r]
 *   PFB_PD_POWER        |Z_c[d][r]|^2, float32, same layout
 *   PFB_PD_BEST         one pfb_mfbank_cell per gate at out[c' R + r]: the largest power over d and the d that gave it.
 *                       The selection walks d = 0, 1, ... and replaces only on a strictly greater power: ties go to
 *                       the lowest d and a power that is not a number never displaces anything (NaN at d = 0 stays):
 *                       the rule of PFB_MFBANK_BEST, and what PFB_CFAR_BANK_CELL reads.
 *   PFB_PD_NONCOHERENT  N_c[r] = sum_k w[k]^2 |A_c[k][r]|^2, float32 at out[c' R + r]: per pulse the windowed sample
 *                       (w re, w im), its squared magnitude, added in float32 for k ascending.
 * PFB_PD_CENTERED (flags): rows are written for d = -ND/2 .. ND/2-1 in that order (row d + ND/2), the hypothesis of a
 * BEST cell is that signed d, and the tie rule walks the signed order.  Row d stands for the pulse-to-pulse frequency
 * d fs / (ND L) (pfb_pd_doppler_frequencies).
 *
 * State: CPI c completes with sample o + ((c+1) K - 1) L + R - 1; cpi_samples = (K-1) L + R is its extent.  A stream
 * may be cut into calls of any length, 0 included.  A CPI that lies wholly inside one call is read where it lies (row
 * stride L, 8-byte alignment).  A CPI that spans calls has its gate samples copied into a device-side K x R carry as
 * they arrive (zeroed when the CPI opens) and is transformed from the carry when it completes; each staging step of a
 * host-pointer call counts as a call here.  Both sources run the same kernel on the same values in the same order, so
 * THE SAME BITS COME OUT UNDER ANY CUTTING of the stream (unlike pfb_mf_*, whose blocks start where calls start).
 * A CPI is taken only if its first sample o + c K L is not before the index the stream (re)started at: create and
 * pfb_pd_reset start at 0, pfb_pd_set_index at its argument.  The carry is K R 8 bytes; more than 64 MiB is
 * PFB_ERR_UNSUPPORTED.  pfb_pd_flush transforms the open CPI with its missing samples as zeros (a no-op when none is
 * open); what the stream brings of that CPI afterwards is ignored.  Lengths outside the set, overlapping CPIs,
 * staggered PRIs, clutter cancellers and integer I/Q input are not built (a PRI that is not a whole number of samples
 * goes through pfb_regrid_* first: the last section of this header).
 *
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers, a wrong
 * struct_size, L, R or K of 0, R > L, K > ND, ND outside the set, L > 2^24, origin > 2^62, an unknown output or flag,
 * a window value that is not finite; per call an unknown mem, a stream index that would pass 2^62, a device pointer
 * not aligned to its element (8 bytes for samples, complex rows, cells and the async count; 4 for float rows).
 * PFB_ERR_UNSUPPORTED: a carry over 64 MiB.  Then PFB_ERR_NO_DEVICE without a HIP device. */
enum { PFB_PD_COMPLEX = 0, PFB_PD_POWER = 1, PFB_PD_BEST = 2, PFB_PD_NONCOHERENT = 3 };
enum { PFB_PD_CENTERED = 1u << 0 };

typedef struct pfb_pd_config {
  uint32_t struct_size;     /* = sizeof(pfb_pd_config)                                          */
  uint32_t pri;             /* L, samples                                                       */
  uint64_t origin;          /* o: stream index of gate 0 of pulse 0                             */
  uint32_t num_gates;       /* R <= L                                                           */
  uint32_t num_pulses;      /* K per CPI                                                        */
  uint32_t doppler_length;  /* ND; 0 = the smallest of the set >= K                             */
  uint32_t output;          /* PFB_PD_*                                                         */
  const float* window;      /* w[0 .. K-1], finite, copied at create; NULL = all ones           */
  uint32_t flags;           /* PFB_PD_CENTERED                                                  */
  int32_t device_id;        /* HIP device ordinal, -1 = current device                          */
} pfb_pd_config;

typedef struct pfb_pd_plan { /* what pfb_pd_describe reports; host only                          */
  uint32_t doppler_length;  /* ND                                                               */
  uint32_t tile_gates;      /* adjacent gates one workgroup takes                               */
  uint64_t carry_bytes;     /* K R 8                                                            */
  uint64_t cpi_samples;     /* (K-1) L + R: from a CPI's first sample to the one completing it  */
  uint64_t cpi_outputs;     /* output elements per CPI: ND R (complex, power), R (best, noncoherent) */
  char kernel[32];          /* the kernel that transforms a CPI                                 */
} pfb_pd_plan;

typedef struct pfb_pd_handle pfb_pd_handle;

/* Host only: validate cfg (everything pfb_pd_create checks before the device) and report the plan. */
int pfb_pd_describe(const pfb_pd_config* cfg, pfb_pd_plan* plan_out);
/* Host only: out[i] = d fs / (ND L) for the ND rows in the order they are written (d = 0 .. ND-1, or -ND/2 .. ND/2-1
 * with PFB_PD_CENTERED).  Reads struct_size, pri, num_pulses, doppler_length and flags of cfg and nothing else.
 * PFB_ERR_BAD_ARG for null pointers, a wrong struct_size, a pri, K or ND pfb_pd_create refuses, or fs not finite. */
int pfb_pd_doppler_frequencies(const pfb_pd_config* cfg, double fs, double* out);
/* Lifecycle as pfb_cfar_*.  The handle owns the window, the twiddles and the carry. */
int pfb_pd_create(const pfb_pd_config* cfg, pfb_pd_handle** out);
int pfb_pd_destroy(pfb_pd_handle* h);
int pfb_pd_reset(pfb_pd_handle* h);   /* drops the open CPI; stream index back to 0 */
int pfb_pd_set_stream(pfb_pd_handle* h, void* hip_stream);
int pfb_pd_sync(pfb_pd_handle* h);
int pfb_pd_get_device(const pfb_pd_handle* h, int* device_id);
/* The CPIs the next num_samples samples complete, given the handle's state now. */
int pfb_pd_cpis_for(const pfb_pd_handle* h, uint64_t num_samples, uint64_t* cpis_out);
int pfb_pd_next_index(const pfb_pd_handle* h, uint64_t* index_out);  /* stream index of the next sample taken */
/* Drops the open CPI and makes next_sample (<= 2^62) the index of the next sample taken (pfb_chsyn_set_frame_index
 * is the precedent). */
int pfb_pd_set_index(pfb_pd_handle* h, uint64_t next_sample);
/* Take num_samples samples; the CPIs they complete go to `out` (room for capacity_cpis CPIs of plan.cpi_outputs
 * elements each) in ascending order, their number to *cpis_out.  PFB_ERR_CAPACITY sets *cpis_out to the number needed
 * and changes no state.  mem: y and out are both host pointers (PFB_MEM_HOST, staged in steps of 2^22 samples; the
 * outputs of one step are held on the device until the step ends) or both device pointers (PFB_MEM_DEVICE).
 * Synchronous.  After PFB_ERR_HIP the stream index is as before the call and the call may be repeated; an open CPI is
 * kept unless the failed call had already closed it and begun another in the carry: then it is dropped, as
 * pfb_pd_set_index(pfb_pd_next_index) would drop it.  What `out` holds after a failure is undefined. */
int pfb_pd_process(pfb_pd_handle* h, const void* y, uint64_t num_samples, void* out, uint64_t capacity_cpis,
                   uint64_t* cpis_out, uint32_t mem);
/* Same, device pointers, enqueued on the handle's stream without a host sync; the number of CPIs the call closed is
 * written to *d_cpis_out, a uint64 in device memory, in stream order.  PFB_ERR_CAPACITY queues nothing. */
int pfb_pd_process_async(pfb_pd_handle* h, const void* d_y, uint64_t num_samples, void* d_out, uint64_t capacity_cpis,
                         uint64_t* d_cpis_out);
/* Transform the open CPI with its missing samples as zeros: *cpis_out is 1, or 0 when none is open.  Capacity
 * contract and mem (of out) as pfb_pd_process. */
int pfb_pd_flush(pfb_pd_handle* h, void* out, uint64_t capacity_cpis, uint64_t* cpis_out, uint32_t mem);
/* The kernel and the source of the last CPI transformed: plan.kernel followed by "[stream]" (read where it lay) or
 * "[carry]"; "" before the first. */
const char* pfb_pd_last_kernel(const pfb_pd_handle* h);

/* ---- PRI search by epoch folding: where pfb_pd_config.pri comes from ----------------------------
 * pfb_pd_* integrates a train whose single pulses are under the detector's threshold, for a caller who knows the PRI to
 * the sample.  The reference carries that number in a script constant (matlab/generate_pulsed_iq.m:16) or on a command
 * line (tx_rx_pulses_usrp.cpp:71); a record off the air carries it nowhere, and a train under the single-pulse threshold
 * leaves pfb_cfar_* no arrival times to difference.  Epoch folding finds it: for each candidate period L the power
 * stream is added into a profile of L / C phase bins.  At the true period every pulse lands in the same bin, which then
 * stands out; at L +- 1 the train walks through the bins and averages away.  This comment is the definition: the device
 * code (csrc/pfb_fold.hip) and the tests' restatement (tests/fold_ref.py) are each written from it.
 *
 * Input: float32 cells p[i] with the global index i = 0, 1, ... since create or reset: what PFB_MF_POWER writes, or any
 * float32 stream.
 * Parameters: bin_cells C (1 .. 64) and a list of NC candidate periods L_c (uint32, copied at create), 1 <= NC <= 4096,
 * each with C <= L <= 2^24 and NB = floor(L / C) <= 65536 bins.  Duplicates are allowed and are separate candidates.
 * The profiles take sum_c NB_c * 4 bytes on the device (plan.profile_bytes); more than 64 MiB is PFB_ERR_UNSUPPORTED.
 *
 * Bin of cell i under period L:  j = min(floor((i mod L) / C), NB - 1).  The L mod C cells left over at the end of a
 * period go into the last bin, which is then C .. 2C-1 cells wide, never narrower (a narrow last bin has few cells
 * behind its mean and wins the maximum on noise alone).
 *
 * Profile: F_L[j] is the float32 sum of the p[i] of bin j, added ONE AT A TIME IN ASCENDING i, starting from +0.0f.
 * No tree, no atomics, no partial sums combined afterwards; only additions occur, so no FMA can arise.  The profile is
 * therefore a function of the cells taken so far: THE SAME BITS COME OUT UNDER ANY CUTTING OF THE STREAM into calls; a
 * call may be empty or end in the middle of a bin of a period.  NaN and Inf go where IEEE addition takes them.
 *
 * Counts, all integers, after N cells:  n_L[j](N) = floor(N / L) (b - a) + clamp((N mod L) - a, 0, b - a)  with a = j C
 * and b = (j + 1) C, or b = L for the last bin (pfb_fold_counts; host only).
 *
 * Score of a candidate after N cells: one pfb_fold_score, in list order (pfb_fold_scores).
 *   m_j = (double)F[j] / (double)n_j, the correctly rounded float64 quotient, for the bins with n_j > 0: the leading
 *   bins_used ones.
 *   The peak walks j ascending and replaces only on a strictly greater m_j: ties go to the lowest j, a NaN never
 *   displaces anything, and a NaN in the first used bin stays -- the rule of PFB_MFBANK_BEST and PFB_PD_BEST.
 *   peak_sum = F[peak_bin], peak_cells = n[peak_bin], peak_mean = (float)m_peak.
 *   sum_means = sum_j m_j and sum_sq_means = sum_j m_j^2 over the used bins, in float64.  THEIR ORDER IS NOT FIXED (a
 *   workgroup reduces them): they are good to (bins_used + 1) 2^-53 sum |terms|, the bound of any-order float64
 *   summation plus the square's rounding.  Every other field is a fixed function of the cells.
 *   With N = 0 every field but period, num_bins and cells is 0.
 * A caller's statistic from these: mu = sum_means / bins_used, z = (peak_mean - mu) / sqrt(sum_sq_means / bins_used -
 * mu^2).  The true period, its multiples and its divisors (if listed) score high; origin = peak_bin * C is, modulo the
 * period, where the train's compressed peak lies (to one bin), and is what pfb_pd_config.origin takes.
 *
 * Not built: splitting one candidate's time axis over workgroups (the order above forbids it), staggered periods, a
 * fast-folding tree that shares additions between candidates, PFB_CFAR_BANK_CELL input, folding fused into the matched
 * filter's store.  Periods that are not whole samples are pfb_qfold_*'s (the last section of this header).
 *
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers (the list
 * included), a wrong struct_size, C outside 1 .. 64, NC outside 1 .. 4096, a period < C or > 2^24 or with more than
 * 65536 bins, flags != 0; per call an unknown mem, a device pointer not aligned to its element (4 bytes for cells and
 * profiles, 8 for score records), an index that would pass 2^62, a candidate >= NC.  Then PFB_ERR_UNSUPPORTED: profiles
 * over 64 MiB.  Then PFB_ERR_NO_DEVICE without a HIP device. */
typedef struct pfb_fold_config {
  uint32_t struct_size;     /* = sizeof(pfb_fold_config)                                        */
  uint32_t bin_cells;       /* C                                                                */
  uint32_t num_periods;     /* NC                                                               */
  const uint32_t* periods;  /* L_c, c = 0 .. NC-1, copied at create                             */
  uint32_t flags;           /* 0                                                                */
  int32_t device_id;        /* HIP device ordinal, -1 = current device                          */
} pfb_fold_config;

typedef struct pfb_fold_plan { /* what pfb_fold_describe reports; host only                      */
  uint64_t profile_bytes;   /* sum_c NB_c * 4 (the handle holds a second copy: pfb_fold_process)*/
  uint64_t total_bins;      /* sum_c NB_c                                                       */
  uint32_t max_bins;        /* max_c NB_c                                                       */
  char kernel[32];          /* the kernel that folds a call                                     */
} pfb_fold_plan;

typedef struct pfb_fold_score {  /* 56 bytes */
  uint32_t period, num_bins;     /* L, NB                                                            */
  uint32_t bins_used;            /* bins with n_j > 0: min(NB, ceil(N / C))                          */
  uint32_t peak_bin, peak_cells; /* the bin of largest mean, ties to the lowest; its n_j             */
  uint32_t reserved;             /* 0 */
  float peak_sum, peak_mean;     /* F[peak_bin]; (float)m_peak                                       */
  double sum_means, sum_sq_means;
  uint64_t cells;                /* N */
} pfb_fold_score;

typedef struct pfb_fold_handle pfb_fold_handle;

/* Host only: validate cfg (everything pfb_fold_create checks before the device) and report the plan. */
int pfb_fold_describe(const pfb_fold_config* cfg, pfb_fold_plan* plan_out);
/* Host only: counts_out[j] = n_L[j](num_cells) for the NB bins of candidate `candidate` of cfg (the closed form above).
 * PFB_ERR_BAD_ARG for a cfg pfb_fold_describe refuses with it, a null counts_out, candidate >= NC, num_cells > 2^62. */
int pfb_fold_counts(const pfb_fold_config* cfg, uint32_t candidate, uint64_t num_cells, uint64_t* counts_out);
/* Lifecycle as pfb_cfar_*.  The handle owns the period list and the profiles. */
int pfb_fold_create(const pfb_fold_config* cfg, pfb_fold_handle** out);
int pfb_fold_destroy(pfb_fold_handle* h);
int pfb_fold_reset(pfb_fold_handle* h);   /* profiles to +0, index to 0 */
int pfb_fold_set_stream(pfb_fold_handle* h, void* hip_stream);
int pfb_fold_sync(pfb_fold_handle* h);
int pfb_fold_get_device(const pfb_fold_handle* h, int* device_id);
int pfb_fold_next_index(const pfb_fold_handle* h, uint64_t* index_out);  /* N: global index of the next cell taken */
/* Fold num_cells cells into every profile.  mem: cells is a host pointer (PFB_MEM_HOST, staged in steps of 2^24 cells)
 * or a device pointer (PFB_MEM_DEVICE, 4-byte aligned, nothing more).  Synchronous.  After PFB_ERR_HIP the profiles and
 * the index are as before the call (the handle keeps the copy that makes this so). */
int pfb_fold_process(pfb_fold_handle* h, const float* cells, uint64_t num_cells, uint32_t mem);
/* Same, device pointer, enqueued on the handle's stream without a host sync. */
int pfb_fold_process_async(pfb_fold_handle* h, const float* d_cells, uint64_t num_cells);
/* Write the NC score records of the cells taken so far to `out` (room for `capacity` records; host memory, or device
 * memory aligned to 8 bytes).  Changes no state and may be called any number of times mid-stream.  PFB_ERR_CAPACITY when
 * capacity < NC: nothing is written.  Synchronous. */
int pfb_fold_scores(pfb_fold_handle* h, pfb_fold_score* out, uint64_t capacity, uint32_t mem);
/* Copy F_L of one candidate, NB floats, to `out` (room for capacity_bins): for plotting and for a caller's own
 * statistics.  PFB_ERR_CAPACITY when capacity_bins < NB.  Changes no state.  Synchronous. */
int pfb_fold_profile(pfb_fold_handle* h, uint32_t candidate, float* out, uint64_t capacity_bins, uint32_t mem);
/* The kernel the last call that took cells launched: plan.kernel; "" before the first. */
const char* pfb_fold_last_kernel(const pfb_fold_handle* h);

/* ---- 2-D CFAR detector over range-Doppler maps -------------------------------------------------
 * pfb_pd_* leaves power maps on the device; this unit turns them into one record per target.  It slides a window over
 * the (Doppler row, gate) plane cell by cell: the noise of a cell is the mean of training cells before and after it in
 * range, over a few Doppler rows around its own; a cell over its threshold is reported when it is the largest of its
 * neighbourhood.  Two trains in one gate on different Doppler rows give two records, and the factor for a false-alarm
 * rate is the plain CA factor for the training cells: with Wd = 0 whatever window pfb_pd_* applied, because training
 * and test cell share a row's statistics; with Wd > 0 a taper correlates adjacent rows, the training cells count for
 * fewer, and the rate rises (DESIGN.md section 22 has measured figures).  On the one-row maps of PFB_PD_NONCOHERENT it
 * is the cell-sliding 1-D detector pfb_cfar_* leaves out.
 * This comment is the definition: the device code (csrc/pfb_rdcfar.hip) and the tests' restatement
 * (tests/rdcfar_ref.py) are each written from it.
 *
 * Input: maps P_m[d][r], float32, m = 0, 1, ... counting maps since create or reset, rows d = 0 .. ND-1 (ND any
 * integer 1 .. 1024), gates r = 0 .. R-1 (R = 1 .. 2^20): the element lies at maps[(m' ND + d) pitch + r], m' the map's
 * place in the call, pitch >= R (0 means R), ND pitch <= 2^26.  Rows are circular (Doppler wraps), gates are not.  The
 * unit does not care in which order the rows stand (PFB_PD_CENTERED or not): it reports the row as stored.
 * Parameters: Doppler half-width Wd (0 .. 16, 2 Wd + 1 <= ND), gate guard Gr (0 .. 1024), gate training per side Tr
 * (1 .. 256), peak half-width in rows Pd (0 .. 16, 2 Pd + 1 <= ND), method (CA, GO, SO: the PFB_CFAR_* values), alpha
 * (float32, finite, > 0), min_power (float32, >= 0).
 *
 * Column sum: A[d][r] is the float64 sum of (double)P[(d + j) mod ND][r] for j = -Wd .. Wd, added ONE AT A TIME IN
 * ASCENDING j, starting from +0.0.
 *
 * Noise of cell (d, r): the lead gates are r-Gr-Tr .. r-Gr-1 that are >= 0 (nL of them), the lag gates r+Gr+1 ..
 * r+Gr+Tr that are < R (nR).  sumL and sumR are float64 sums of A[d][.] over those gates, one at a time in ascending
 * gate, each starting from +0.0.
 *   CA  noise = (float)((sumL + sumR) / ((nL + nR) (2 Wd + 1)))
 *   GO  noise = (float)max(sumL / (nL (2 Wd + 1)), sumR / (nR (2 Wd + 1)))       SO: the same with min
 * In GO and SO an empty side is left out, and a NaN on either side gives NaN.  All divisions are float64, with one
 * rounding to float32 at the end.  With nL = nR = 0 the cell has no noise: it is never over, and it is counted in
 * pfb_rdcfar_stats.cells_without_noise.
 *
 * Decision: over = (p > alpha * noise) && (p > min_power), p = P[d][r], the product one float32 multiply, as in
 * pfb_cfar_*.  A NaN on either side of a comparison never detects; nothing is special-cased.
 *
 * Detection: an over cell is reported iff no cell of its peak box beats it.  The box is the rows d-Pd .. d+Pd
 * (circular) by the gates r-Gr .. r+Gr (clipped to 0 .. R-1).  q beats p iff P_q > P_p, or P_q == P_p and q's (row,
 * gate), the row as stored, is lower in row-major order.  A NaN neighbour beats nothing.  One pfb_rdcfar_det per
 * reported cell, written in ascending (map, row, gate).
 *
 * Invariance: every figure is a function of one map, so ANY CUTTING OF A SEQUENCE OF MAPS INTO CALLS GIVES THE SAME
 * BYTES.  Only additions, one division and one multiply occur, in the order stated: no atomics, no running sums, no
 * arrival-order compaction (the records are placed by counts and a scan).
 *
 * Cost: a cell walks its 2 Tr training sums itself, and an over cell walks its whole peak box, (2 Pd + 1)(2 Gr + 1)
 * cells, in one lane: correct, and slow only for maps that are all detections.  A call is worked in steps of whole
 * maps, of at most 2^24 cells and 2^18 words of 64 gates (at least one map); a host-pointer call stages its maps in
 * those steps.
 *
 * Not built: guard rows in Doppler, joining adjacent reported cells into 2-D runs, a detector fused into
 * pfb_pd_*'s store.  (OS-CFAR is the unit of its own below, pfb_oscfar_*: DESIGN.md section 23.)
 *
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers, a wrong
 * struct_size, rows outside 1 .. 1024, gates outside 1 .. 2^20, a pitch that is neither 0 nor >= gates or with
 * rows pitch > 2^26, doppler_half_width > 16 or 2 Wd + 1 > rows, guard_gates > 1024, train_gates outside 1 .. 256,
 * peak_half_width > 16 or 2 Pd + 1 > rows, an unknown method, an alpha that is not finite or <= 0, a min_power that is
 * negative or NaN, flags != 0; per call an unknown mem, num_maps > 2^40, capacity > 2^56, a device pointer not aligned
 * to its element (4 bytes for maps, 8 for records and the async count).  Then PFB_ERR_NO_DEVICE without a HIP device. */
#define PFB_RDCFAR_DET_ONE_SIDED 1u /* pfb_rdcfar_det.flags: the cell trained on fewer than 2 Tr gates */

typedef struct pfb_rdcfar_config {
  uint32_t struct_size;         /* = sizeof(pfb_rdcfar_config)                                  */
  uint32_t rows;                /* ND                                                           */
  uint32_t gates;               /* R                                                            */
  uint32_t pitch;               /* floats from one row to the next; 0 = gates                   */
  uint32_t doppler_half_width;  /* Wd                                                           */
  uint32_t guard_gates;         /* Gr                                                           */
  uint32_t train_gates;         /* Tr, per side                                                 */
  uint32_t peak_half_width;     /* Pd                                                           */
  uint32_t method;              /* PFB_CFAR_CA / GO / SO                                        */
  float alpha;
  float min_power;
  uint32_t flags;               /* 0                                                            */
  int32_t device_id;            /* -1 = the current device                                      */
} pfb_rdcfar_config;

typedef struct pfb_rdcfar_plan { /* what pfb_rdcfar_describe reports; host only                  */
  uint64_t training_cells;  /* 2 Tr (2 Wd + 1): what a cell away from the gate edges trains on  */
  uint32_t tile_rows;       /* the band of rows and ...                                         */
  uint32_t tile_gates;      /* ... the tile of gates one workgroup takes                        */
  uint32_t lds_bytes;       /* of one workgroup                                                 */
  uint32_t reserved;        /* 0 */
  char kernel[32];          /* the kernel that decides the cells                                */
} pfb_rdcfar_plan;

typedef struct pfb_rdcfar_det {  /* 32 bytes */
  uint64_t map;                  /* m, since create or reset                                     */
  uint32_t row, gate;            /* d as stored, r                                               */
  float power, noise;            /* P[d][r]; the cell's noise                                    */
  uint32_t training_cells;       /* (nL + nR) (2 Wd + 1)                                         */
  uint32_t flags;                /* PFB_RDCFAR_DET_ONE_SIDED: nL + nR < 2 Tr                     */
} pfb_rdcfar_det;

typedef struct pfb_rdcfar_stats {
  uint64_t maps_in;             /* maps taken since create or reset                              */
  uint64_t cells_over;
  uint64_t cells_without_noise; /* cells with nL = nR = 0                                        */
  uint64_t detections;          /* reported cells, the dropped ones included                     */
  uint64_t dropped;             /* records pfb_rdcfar_process_async had no room to write         */
} pfb_rdcfar_stats;

typedef struct pfb_rdcfar_handle pfb_rdcfar_handle;

/* Host only: validate cfg (everything pfb_rdcfar_create checks before the device) and report the plan. */
int pfb_rdcfar_describe(const pfb_rdcfar_config* cfg, pfb_rdcfar_plan* plan_out);
/* Lifecycle as pfb_cfar_*.  pfb_cfar_alpha(pfa, 2 Tr (2 Wd + 1)) is the CA factor for a false-alarm rate. */
int pfb_rdcfar_create(const pfb_rdcfar_config* cfg, pfb_rdcfar_handle** out);
int pfb_rdcfar_destroy(pfb_rdcfar_handle* h);
int pfb_rdcfar_reset(pfb_rdcfar_handle* h);   /* map index back to 0, stats zeroed */
int pfb_rdcfar_set_stream(pfb_rdcfar_handle* h, void* hip_stream);
int pfb_rdcfar_sync(pfb_rdcfar_handle* h);
int pfb_rdcfar_get_device(const pfb_rdcfar_handle* h, int* device_id);
int pfb_rdcfar_next_map(const pfb_rdcfar_handle* h, uint64_t* map_out);  /* m of the next map taken */
/* Synchronises the handle's stream: the device keeps the counts that depend on the data. */
int pfb_rdcfar_get_stats(pfb_rdcfar_handle* h, pfb_rdcfar_stats* stats_out);
/* Take num_maps maps and write their detections, in order, to det_out (room for `capacity`); their number goes to
 * *count_out.  PFB_ERR_CAPACITY sets *count_out to the number needed and changes no state (what det_out holds is then
 * unspecified).  mem: maps and det_out are both host pointers (PFB_MEM_HOST) or both device pointers
 * (PFB_MEM_DEVICE).  Synchronous. */
int pfb_rdcfar_process(pfb_rdcfar_handle* h, const float* maps, uint64_t num_maps, pfb_rdcfar_det* det_out,
                       uint64_t capacity, uint64_t* count_out, uint32_t mem);
/* Device pointers, enqueued on the handle's stream without a host sync.  *d_count_out (a uint64 in device memory) is
 * the number of detections of the call.  The first `capacity` records in order are written; the rest are counted in
 * pfb_rdcfar_stats.dropped, and the state advances. */
int pfb_rdcfar_process_async(pfb_rdcfar_handle* h, const float* d_maps, uint64_t num_maps, pfb_rdcfar_det* d_det_out,
                             uint64_t capacity, uint64_t* d_count_out);
/* Host only: detections as pulse descriptor words, so that pfb_event_fit takes them as it takes PDWs.  The maps are
 * those of a pfb_pd_* with these pri, num_pulses and origin; `rows` is its ND and `centered` whether it wrote its rows
 * with PFB_PD_CENTERED.  The signed bin of row d is d - floor(ND / 2) when centered, else d for d < ceil(ND / 2) and
 * d - ND above.
 *   toa = (origin + map * num_pulses * pri + gate + 1) / fs + sample_start_time: the train's first pulse of that
 *   interval (pulse 0), in the extractors' 1-based convention
 *   freq = fc + signed_bin * fs / (rows * pri)      bin = signed_bin
 *   pw = 1 / fs      snr = 10 log10(power / noise)      mag = sqrt(power)      sat = 0
 * PFB_ERR_BAD_ARG for null pointers (with n > 0), an fs that is not finite and > 0, a pri, num_pulses or rows of 0, or
 * a record whose row is >= rows. */
int pfb_rdcfar_to_pdw(const pfb_rdcfar_det* dets, uint64_t n, double fs, double fc, double sample_start_time,
                      uint32_t pri, uint32_t num_pulses, uint64_t origin, uint32_t rows, uint32_t centered,
                      pfb_pdw* pdw_out);
/* The kernel the last call that took maps launched: plan.kernel; "" before the first. */
const char* pfb_rdcfar_last_kernel(const pfb_rdcfar_handle* h);

/* ---- ordered-statistic CFAR over range-Doppler maps --------------------------------------------
 * Every other detector here estimates a cell's noise as a mean, and a mean breaks when a second target stands in the
 * training window: the interferer raises it and the weaker target disappears.  This unit takes the k-th smallest of
 * the training cells instead (OS-CFAR): up to N - k interferers in a window leave the estimate where it was.  Input,
 * geometry, decision, peak box, records (pfb_rdcfar_det, PFB_RDCFAR_DET_ONE_SIDED), stats (pfb_rdcfar_stats),
 * capacity and async semantics are pfb_rdcfar_*'s; pfb_rdcfar_to_pdw takes its records unchanged.
 * This comment is the definition: the device code (csrc/pfb_oscfar.hip) and the tests' restatement
 * (tests/oscfar_ref.py) are each written from it.
 *
 * Input: maps P_m[d][r], float32, exactly as pfb_rdcfar_*: rows d = 0 .. ND-1 (1 .. 1024) are circular, gates r = 0 ..
 * R-1 (1 .. 2^20) are not; the element lies at maps[(m' ND + d) pitch + r], pitch >= R (0 means R), ND pitch <= 2^26.
 * Parameters: Wd (0 .. 16, 2 Wd + 1 <= ND), Gr (0 .. 1024), Tr (1 .. 256), Pd (0 .. 16, 2 Pd + 1 <= ND), alpha (float32,
 * finite, > 0), min_power (float32, >= 0), and the rank k = 1 .. N, where N = 2 Tr (2 Wd + 1) is what a cell away from
 * the gate edges trains on.  N must be <= 4096.
 *
 * Training set of cell (d, r): the values P[(d + j) mod ND][g] for j = -Wd .. Wd and g over the lead gates r-Gr-Tr ..
 * r-Gr-1 that are >= 0 (nL of them) and the lag gates r+Gr+1 .. r+Gr+Tr that are < R (nR): n = (nL + nR)(2 Wd + 1)
 * values.  With n = 0 the cell has no noise: it is never over, and it is counted in
 * pfb_rdcfar_stats.cells_without_noise.
 *
 * Rank at the gate edges: k' = ceil(k n / N), in integers (k n + N - 1) / N: k' = k for a fully trained cell and
 * 1 <= k' <= n otherwise.  The record's training_cells = n and PFB_RDCFAR_DET_ONE_SIDED (nL + nR < 2 Tr) tell which.
 *
 * Noise of the cell: the k'-th smallest training value under float32 `<`, where a NaN ranks after every number and
 * -0 and +0 are equal.  Equivalently the smallest training value v with #{x_i <= v} >= k'; when there is none (fewer
 * than k' values are numbers), the noise is NaN.  A zero is reported as +0.0, so the bytes are unique.  A NaN noise
 * never detects, and the cell is NOT counted in cells_without_noise.
 *
 * Decision: over = (p > alpha * noise) && (p > min_power), p = P[d][r], the product one float32 multiply.  Because
 * alpha > 0 and a float32 multiply is monotone, p > alpha * noise holds exactly when at least k' training values
 * satisfy alpha * x_i < p (a NaN compares false): an implementation may decide by counting and select the noise only
 * for the cells that are over.
 *
 * Detection, peak box, ties and record order: pfb_rdcfar_*'s, word for word.  The box is the rows d-Pd .. d+Pd
 * (circular) by the gates r-Gr .. r+Gr (clipped); q beats p iff P_q > P_p, or P_q == P_p and q's (row, gate) is lower
 * in row-major order; a NaN neighbour beats nothing.  One pfb_rdcfar_det per reported cell (noise: the order
 * statistic), in ascending (map, row, gate).
 *
 * Invariance: every figure is a function of one map, so ANY CUTTING OF A SEQUENCE OF MAPS INTO CALLS GIVES THE SAME
 * BYTES.  The noise is a rank, not a sum: THE ORDER IN WHICH THE TRAINING CELLS ARE VISITED IS FREE, and a sliding or
 * shared evaluation is allowed.  No atomics; the records are placed by counts and a scan.
 *
 * Cost: a cell reads at most its n training values once to decide; an over cell has them read 32 times more to select
 * its noise (a bitwise search on an order-preserving integer key, shared out over its wave) and walks its peak box in
 * one lane: slow only for maps that are all detections.  Steps and host staging as pfb_rdcfar_*.
 *
 * pfb_oscfar_alpha: for independent exponentially distributed cells (power of complex Gaussian noise) the k-th of N
 * gives P(over) = prod_{i=0}^{k-1} (N - i) / (N - i + alpha); the factor is the root of that product = pfa.
 *
 * Not built: OS in the block detector pfb_cfar_*, trimmed or censored means, guard rows in Doppler, a detector fused
 * into pfb_pd_*'s store.
 *
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers, a wrong
 * struct_size, rows outside 1 .. 1024, gates outside 1 .. 2^20, a pitch that is neither 0 nor >= gates or with
 * rows pitch > 2^26, doppler_half_width > 16 or 2 Wd + 1 > rows, guard_gates > 1024, train_gates outside 1 .. 256,
 * peak_half_width > 16 or 2 Pd + 1 > rows, N = 2 Tr (2 Wd + 1) > 4096, a rank outside 1 .. N, an alpha that is not
 * finite or <= 0, a min_power that is negative or NaN, flags != 0; per call an unknown mem, num_maps > 2^40,
 * capacity > 2^56, a device pointer not aligned to its element (4 bytes for maps, 8 for records and the async count).
 * Then PFB_ERR_NO_DEVICE without a HIP device. */
typedef struct pfb_oscfar_config {
  uint32_t struct_size;         /* = sizeof(pfb_oscfar_config)                                  */
  uint32_t rows;                /* ND                                                           */
  uint32_t gates;               /* R                                                            */
  uint32_t pitch;               /* floats from one row to the next; 0 = gates                   */
  uint32_t doppler_half_width;  /* Wd                                                           */
  uint32_t guard_gates;         /* Gr                                                           */
  uint32_t train_gates;         /* Tr, per side                                                 */
  uint32_t peak_half_width;     /* Pd                                                           */
  uint32_t rank;                /* k = 1 .. 2 Tr (2 Wd + 1)                                     */
  float alpha;
  float min_power;
  uint32_t flags;               /* 0                                                            */
  int32_t device_id;            /* -1 = the current device                                      */
} pfb_oscfar_config;

typedef struct pfb_oscfar_plan { /* what pfb_oscfar_describe reports; host only                  */
  uint64_t training_cells;  /* N = 2 Tr (2 Wd + 1)                                              */
  uint32_t tile_rows;       /* the band of rows and ...                                         */
  uint32_t tile_gates;      /* ... the tile of gates one workgroup takes                        */
  uint32_t lds_bytes;       /* of one workgroup; 0 when the maps are read through the caches    */
  uint32_t reserved;        /* 0 */
  char kernel[32];          /* the kernel that decides the cells                                */
} pfb_oscfar_plan;

typedef struct pfb_oscfar_handle pfb_oscfar_handle;

/* Host only: validate cfg (everything pfb_oscfar_create checks before the device) and report the plan. */
int pfb_oscfar_describe(const pfb_oscfar_config* cfg, pfb_oscfar_plan* plan_out);
/* Host only: the factor alpha for a false-alarm rate pfa with rank k of N training cells, solved in float64 by
 * bisection on the logarithm of the product above.  PFB_ERR_BAD_ARG for a null pointer, a pfa outside (0, 1),
 * training_cells = 0 or > 2^20, or a rank outside 1 .. training_cells. */
int pfb_oscfar_alpha(double pfa, uint64_t training_cells, uint64_t rank, double* alpha_out);
/* Lifecycle, calls and stats as pfb_rdcfar_*. */
int pfb_oscfar_create(const pfb_oscfar_config* cfg, pfb_oscfar_handle** out);
int pfb_oscfar_destroy(pfb_oscfar_handle* h);
int pfb_oscfar_reset(pfb_oscfar_handle* h);   /* map index back to 0, stats zeroed */
int pfb_oscfar_set_stream(pfb_oscfar_handle* h, void* hip_stream);
int pfb_oscfar_sync(pfb_oscfar_handle* h);
int pfb_oscfar_get_device(const pfb_oscfar_handle* h, int* device_id);
int pfb_oscfar_next_map(const pfb_oscfar_handle* h, uint64_t* map_out);  /* m of the next map taken */
/* Synchronises the handle's stream: the device keeps the counts that depend on the data. */
int pfb_oscfar_get_stats(pfb_oscfar_handle* h, pfb_rdcfar_stats* stats_out);
/* As pfb_rdcfar_process: PFB_ERR_CAPACITY sets *count_out to the number needed and changes no state.  Synchronous. */
int pfb_oscfar_process(pfb_oscfar_handle* h, const float* maps, uint64_t num_maps, pfb_rdcfar_det* det_out,
                       uint64_t capacity, uint64_t* count_out, uint32_t mem);
/* As pfb_rdcfar_process_async: device pointers, no host sync; what does not fit is counted in stats.dropped. */
int pfb_oscfar_process_async(pfb_oscfar_handle* h, const float* d_maps, uint64_t num_maps, pfb_rdcfar_det* d_det_out,
                             uint64_t capacity, uint64_t* d_count_out);
/* The kernel the last call that took maps launched: plan.kernel; "" before the first. */
const char* pfb_oscfar_last_kernel(const pfb_oscfar_handle* h);

/* ---- PDW deinterleaver: emitters from arrival times ---------------------------------------------
 * Every detector here ends in one time-ordered table of pulses; a record off the air holds several emitters whose
 * pulses arrive interleaved.  This unit takes the table apart: a difference histogram of the arrival times proposes
 * periods, a sequence search pulls the train of the best one out, and the rest goes round again until nothing is
 * left.  pfb_fold_* finds the period of a train too weak to give arrival times; this unit is for pulses that have them.
 * Every figure is an integer (one IEEE division apart), so the results are bytes, not tolerances.
 * This comment is the definition: the device code (csrc/pfb_deint.hip) and the tests' restatement
 * (tests/deint_ref.py) are each written from it.
 *
 * Input: t[0 .. N), uint64 arrival ticks in non-decreasing order (duplicates allowed), N <= 2^20, every tick < 2^62,
 * in host or device memory by `mem` (a device pointer is 8-byte aligned).  A tick is the caller's clock: the
 * peak_index of a pfb_cfar_det, a PDW's toa turned into frames (pfb_deint_ticks_from_toa).
 *
 * Parameters: pmin = min_period, pmax = max_period (1 <= pmin <= pmax <= 2^31), W = bin_ticks (>= 1, with NB =
 * (pmax - pmin) / W + 1 <= 65536 bins), Lv = max_level (1 .. 256), detect_percent (1 .. 100), min_pulses (3 .. 2^20),
 * X = max_missing (0 .. 8), e = tolerance (0 means W; e (2 X + 3) < pmin keeps the X + 1 search windows of one pulse
 * apart), fill_percent (1 .. 100), max_emitters (1 .. 1024).
 *
 * A round works on the ALIVE pulses, those not yet assigned, in their order: a[0 .. n), a[q] = t[idx[q]].
 *  1. Histogram: every pair (i, j) with 1 <= j - i <= Lv and d = a[j] - a[i] in [pmin, pmax] adds 1 to
 *     C[(d - pmin) / W], C uint32.  A count of a set: the order is free.
 *  2. Candidates, k ascending, a missing neighbour taken as 0: bin k is a candidate iff C[k] > C[k-1], C[k] >= C[k+1]
 *     and S_k = C[k-1] + C[k] + C[k+1] >= max(min_pulses - 1, ceil(floor(span / tau_k) detect_percent / 100)), with
 *     tau_k = pmin + k W + W / 2 (integer division) and span = a[n-1] - a[0].  Ascending order is the subharmonic
 *     rule: the bin at 2 tau is reached only after tau has been tried and its train removed.
 *  3. Successor of alive pulse i at period tau: for m = 0 .. X in turn the target is a[i] + (m + 1) tau and the window
 *     target -+ (m + 1) e, inclusive.  Among the alive j > i inside the window the one with the smallest
 *     |a[j] - target| is taken, ties to the lowest j.  The first m that finds one gives succ(i) = j, step(i) = m + 1;
 *     if none does there is no successor.
 *  4. Chains: len(i) = 1 + len(succ(i)), per(i) = step(i) + per(succ(i)), end(i) = end(succ(i)); without a successor
 *     1, 0 and i.  The best start b is the i of largest len, ties to the lowest i.  The candidate is ACCEPTED iff
 *     len(b) >= min_pulses and 100 (len(b) - 1) >= fill_percent per(b): the fill rule refuses the sparse chains that
 *     a fraction of a real period strings together through the miss windows.  A refused candidate gives way to the
 *     next one of the same histogram.
 *  5. Extraction: the pulses of b's chain get label E, the index of the record, and leave the alive set; one
 *     pfb_deint_emitter is written; the next round begins with a new histogram.
 * The run ends when fewer than min_pulses pulses are alive (no histogram is built then), when no candidate of a
 * round is accepted, or when max_emitters records exist.
 *
 * Output: labels, int32, one per input pulse, -1 for unassigned; records in extraction order.  Both are pure
 * functions of the list and the config: THE SAME CALL TWICE, AND HOST AND DEVICE INPUT, GIVE THE SAME BYTES.  Integer
 * adds commute, so the histogram may use integer atomics; there are no float atomics.
 *
 * Stats of the last run: rounds = histograms built, candidates_tried = successor searches made, candidates_refused =
 * those not accepted, pulses_assigned = the sum of the records' pulses.
 *
 * Tiers.  Histogram: a workgroup stages tiles of 1024 consecutive alive ticks plus Lv more in LDS and its lanes take
 * (i, level) pairs; for NB <= 8192 (pfb_deint_plan.lds_bins) it counts in a private LDS histogram that it adds to the
 * global one once (pfb_deint_hist_lds), above that straight into the global one (pfb_deint_hist_global).  Successors:
 * one lane per alive pulse (pfb_deint_succ).  Chains: pointer doubling over (succ, len, per), an argmax and a marking
 * pass that reads the kept jump tables of the doubling rounds (pfb_deint_mark_tables) or, by pfb_deint_set_tier, walks
 * b's chain in one lane (pfb_deint_mark_walk).  pfb_deint_last_kernel joins the names of what the last call launched with '+'.
 *
 * Not built: an async form (the decision of every round returns to the host), staggered, jittered-by-design or
 * sliding PRIs, frequency or pulse-width clustering inside this unit (pfb_cluster_* splits the list first), a
 * streaming form over PDW chunks, the PRI transform's phase weighting, a histogram fused into the detectors' emit.
 *
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers, a wrong
 * struct_size, min_period = 0, max_period < min_period or > 2^31, bin_ticks = 0, NB > 65536, max_level outside
 * 1 .. 256, detect_percent outside 1 .. 100, min_pulses outside 3 .. 2^20, max_missing > 8, e (2 X + 3) >= pmin,
 * fill_percent outside 1 .. 100, max_emitters outside 1 .. 1024, flags != 0; per call a null handle, an unknown mem,
 * n > 2^20, a null ticks with n > 0, a null output (labels_out may be null only with n = 0), a device pointer not
 * aligned to its element (8 bytes for ticks and records, 4 for labels, counts and the successor arrays), and for
 * pfb_deint_successors a period outside 1 .. 2^32 - 1 or with e (2 X + 3) >= period.  PFB_ERR_CAPACITY: capacity_bins
 * < NB.  Then PFB_ERR_NO_DEVICE without a HIP device.  The order of the ticks and their bound 2^62 are checked on the
 * device, in the first pass over the list: a list that fails returns PFB_ERR_BAD_ARG with nothing written. */
typedef struct pfb_deint_config {
  uint32_t struct_size;     /* = sizeof(pfb_deint_config)                                       */
  uint32_t min_period;      /* pmin, ticks                                                      */
  uint32_t max_period;      /* pmax                                                             */
  uint32_t bin_ticks;       /* W                                                                */
  uint32_t max_level;       /* Lv: differences up to the Lv-th neighbour                        */
  uint32_t detect_percent;  /* of the span / tau pairs a full train would give                  */
  uint32_t min_pulses;      /* of a train                                                       */
  uint32_t max_missing;     /* X: pulses in a row a chain may step over                         */
  uint32_t tolerance;       /* e, ticks per period stepped; 0 = W                               */
  uint32_t fill_percent;    /* hits per period a chain must reach                               */
  uint32_t max_emitters;    /* records after which the run ends                                 */
  uint32_t flags;           /* 0                                                                */
  int32_t device_id;        /* -1 = the current device                                          */
} pfb_deint_config;

typedef struct pfb_deint_plan { /* what pfb_deint_describe reports; host only                     */
  uint64_t scratch_bytes;     /* device memory a handle holds after pfb_deint_run on n pulses     */
  uint32_t num_bins;          /* NB                                                               */
  uint32_t lds_bins;          /* the largest NB the LDS tier takes                                */
  uint32_t tile_pulses;       /* alive pulses of one histogram tile (Lv more are staged)          */
  uint32_t lds_bytes;         /* of one histogram workgroup                                       */
  uint32_t successor_threads; /* lanes of one workgroup of the successor kernel                   */
  uint32_t reserved;          /* 0 */
  char histogram_kernel[32];
  char successor_kernel[32];
  char marking_kernel[32];
} pfb_deint_plan;

typedef struct pfb_deint_emitter {  /* 48 bytes */
  uint64_t first_tick;        /* a[b]                                                             */
  uint64_t last_tick;         /* a[end(b)]                                                        */
  double period;              /* (double)(last_tick - first_tick) / (double)periods: one division */
  uint32_t pulses;            /* len(b)                                                           */
  uint32_t periods;           /* per(b): periods from the first pulse to the last                 */
  uint32_t bin;               /* k of the candidate                                               */
  uint32_t candidate_period;  /* tau_k                                                            */
  uint32_t first_pulse;       /* index of the first pulse in the caller's list                    */
  uint32_t hist_count;        /* S_k                                                              */
} pfb_deint_emitter;

typedef struct pfb_deint_stats {
  uint64_t rounds;
  uint64_t candidates_tried;
  uint64_t candidates_refused;
  uint64_t pulses_assigned;
} pfb_deint_stats;

typedef struct pfb_deint_handle pfb_deint_handle;

/* Host only: validate cfg (everything pfb_deint_create checks before the device) and report the plan for a list of
 * n pulses (n > 2^20: PFB_ERR_BAD_ARG). */
int pfb_deint_describe(const pfb_deint_config* cfg, uint64_t n, pfb_deint_plan* plan_out);
/* Lifecycle as pfb_fold_*.  The scratch grows with the longest list seen and is kept. */
int pfb_deint_create(const pfb_deint_config* cfg, pfb_deint_handle** out);
int pfb_deint_destroy(pfb_deint_handle* h);
int pfb_deint_set_stream(pfb_deint_handle* h, void* hip_stream);
int pfb_deint_sync(pfb_deint_handle* h);
int pfb_deint_get_device(const pfb_deint_handle* h, int* device_id);
/* The whole search.  emitters_out (capacity records) and labels_out (n int32) are host memory, or device memory with
 * mem = PFB_MEM_DEVICE; *count_out (host) is the number of records found.  PFB_ERR_CAPACITY when that is more than
 * capacity: *count_out holds the true count, neither array is written and the stats stay those of the run before.
 * Synchronous. */
int pfb_deint_run(pfb_deint_handle* h, const uint64_t* ticks, uint64_t n, uint32_t mem, pfb_deint_emitter* emitters_out,
                  uint64_t capacity, uint64_t* count_out, int32_t* labels_out);
/* Step 1 alone on the whole list: NB uint32 counts, for plots and for the tests.  Changes no stats. */
int pfb_deint_histogram(pfb_deint_handle* h, const uint64_t* ticks, uint64_t n, uint32_t mem, uint32_t* counts_out,
                        uint64_t capacity_bins);
/* Steps 3 and 4 alone on the whole list at one period: succ(i) (-1 for none), step(i) (0 for none) and len(i), n
 * int32 each.  Changes no stats. */
int pfb_deint_successors(pfb_deint_handle* h, const uint64_t* ticks, uint64_t n, uint32_t mem, uint64_t period,
                         int32_t* succ_out, int32_t* step_out, int32_t* len_out);
/* The kernels the last call launched, joined with '+'; "" before the first and after a call that launched none. */
const char* pfb_deint_last_kernel(const pfb_deint_handle* h);
/* The stats of the last pfb_deint_run that returned PFB_OK; zeros before the first. */
int pfb_deint_get_stats(const pfb_deint_handle* h, pfb_deint_stats* stats_out);
/* Host only: tick = llrint((toa - t0) tick_rate) of the n doubles at toa, stride_bytes apart (8 for a plain array,
 * sizeof(pfb_pdw) to walk a pfb_pdw array's toa field in place), sorted ascending and stably: ticks_out[i] is the tick
 * of element order_out[i].  PFB_ERR_BAD_ARG for null pointers, stride_bytes < 8, n > 2^31, a tick_rate that is not
 * finite or <= 0, a t0 that is not finite, a toa that is not finite, a negative tick or one >= 2^62; nothing is
 * written then. */
int pfb_deint_ticks_from_toa(const double* toa, uint64_t stride_bytes, uint64_t n, double t0, double tick_rate,
                             uint64_t* ticks_out, uint32_t* order_out);

/* ---- Modulation on pulse: what is inside a pulse -------------------------------------------------
 * The detectors say where a pulse is; pfb_pdw.freq says one median phase step about its inside, so a chirp comes back
 * as its mid frequency and a phase code as a carrier.  This unit measures, per pulse of a list, a handful of sums of
 * lag products over the pulse's samples: the mean phase step (mid frequency), the sweep, and the phase flips of a code.
 * For the integer formats every sum is an exact integer, so any order of summation gives THE SAME BYTES.
 * This comment is the definition: the device code (csrc/pfb_mop.hip) and the tests' restatement (tests/mop_ref.py)
 * are each written from it.
 *
 * Input: a series x of num_samples rows.  PFB_FMT_INT8_IQ / PFB_FMT_INT16_IQ: interleaved I,Q integers, ld = 1, the
 * sums in counts (not normalised; bit_width is checked and otherwise unused).  PFB_FMT_CF32: complex float32 with a
 * pitch: element i of column c is x[i ld + c], 1 <= ld, c < ld -- a column of pfb_process's frame-major matrix is
 * measured where it lies, and so is a plain cf32 stream (ld = 1).  base_index is the global index of row 0.  A list
 * of num_pulses pfb_mop_pulse in any order; overlapping and duplicate pulses are allowed; start is a global index.
 *
 * Per pulse, with t = trim_samples: n = min(length - 2t, 2^20), or 0 when length <= 2t; u[i] is element
 * start - base_index + t + i, i = 0 .. n-1, u = I + jQ, the components int64 for the integer formats and converted
 * to double for cf32.  EVERY EXPRESSION BELOW IS EVALUATED AS WRITTEN, one IEEE operation at a time, no contraction
 * into fused multiply-adds, so that a float64 restatement gets the same bits for every term.
 *   z1[i] = u[i+1] conj(u[i]):  a[i] = I[i+1] I[i] + Q[i+1] Q[i],  b[i] = Q[i+1] I[i] - I[i+1] Q[i],  i = 0 .. n-2
 *   S1 = sum (a[i], b[i]): its argument is the mean phase step, for a symmetric sweep the mid frequency
 *   L = (n - 1) / 2 (integer division)
 *   S2 = sum over i = 0 .. n-2-L of z1[i+L] conj(z1[i]):  re = a[i+L] a[i] + b[i+L] b[i],  im = b[i+L] a[i] - a[i+L] b[i]
 *        its argument is 2 pi rate L / fs^2, unambiguous for every sweep under fs because L <= (n-1)/2.  A lag of 1
 *        instead has a per-term phase of 2 pi extent / (n fs), which drowns in noise: hence the half-length lag.
 *   c[i] = a[i+1] a[i] + b[i+1] b[i], i = 0 .. n-3: the real part of the lag-1 second-order product.  neg_count = the
 *        number of i with c[i] < 0 (a NaN is not < 0); first_neg / last_neg the lowest / highest such i, 0xFFFFFFFF
 *        when there is none.  The first max_negatives such i go in ascending order to the optional side array
 *        negs_out[p max_negatives + j] (uint32), the entries of a pulse past its count 0xFFFFFFFF;
 *        negs_listed = min(neg_count, max_negatives), whether or not negs_out is given.
 *   energy = sum (I^2 + Q^2); peak_power the largest I^2 + Q^2 and peak_index its lowest i.  A NaN never wins; with no
 *        winner peak_index = 0xFFFFFFFF and peak_power = 0.
 * Empty sums are +0.
 *
 * Exactness.  Integer formats: exact integer arithmetic.  a, b and the terms of S2 stay within +-2^62 (Cauchy-Schwarz
 * at int16 full scale); S1 and energy stay under 2^53 and are reported exactly.  An S2 sum needs up to 82 bits: it is
 * accumulated in two limbs, the terms' signed high 32 bits (term >> 32, arithmetic) and unsigned low 32 bits, each in
 * an int64 (safe for n <= 2^20), and reported as ldexp((double)hi, 32) + (double)lo, the float64 nearest the exact
 * sum, one rounding.  No order of summation is prescribed because none matters.  cf32: the terms are the float64
 * values above, summed in the fixed order of the kernel that takes the pulse: THE SAME CALL TWICE GIVES THE SAME
 * BYTES; each sum is within (n + 4) 2^-53 sum m_i of the exact one, m_i the sum of the magnitudes of a term's two
 * products.  There are no floating-point atomics; the integer atomics only build work lists.
 *
 * Output: one 96-byte pfb_mop_record per pulse in the caller's order.  Flags: PFB_MOP_OUTSIDE: [start, start+length)
 * is not wholly inside [base_index, base_index + num_samples), or column >= ld; then n = 0 and everything else is
 * zero / 0xFFFFFFFF.  PFB_MOP_SHORT: n < 3 (an OUTSIDE pulse is SHORT too).  PFB_MOP_TRUNCATED: length - 2t > 2^20.
 * PFB_MOP_NEGS_CLIPPED: neg_count > max_negatives.
 *
 * Tiers, by n (pfb_mop_plan): mop_wave, one wave per pulse, four pulses to a workgroup, for n < group_min; mop_group,
 * one workgroup per pulse, each wave a quarter of it, for n < split_min; mop_split + mop_join, the pulse cut into
 * parts of part_samples for as many workgroups, whose partial sums (integers, or doubles in part order) and first
 * max_negatives negatives a second small kernel joins, from split_min on.  Lanes take consecutive i, so every load is
 * coalesced.  The grid is capped at grid_cap workgroups, which loop over their units of work.  pfb_mop_measure_async
 * cannot read how many pulses are long and keeps them on mop_group.  pfb_mop_last_kernel joins what ran with '+'.
 *
 * Host route: with x in host memory only the pulses' windows are uploaded, packed back to back into a page-locked
 * staging buffer, a batch of whole pulses at a time, and the same kernels run on the packed windows: the bytes equal
 * the device route's, the records echo the caller's start / length / column.
 *
 * Not built: the measurement inside the deinterleaver, polyphase codes (more than two phases), nonlinear sweeps.
 *
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers or a wrong
 * struct_size, max_negatives > 128, trim_samples > 2^19; then PFB_ERR_BAD_FORMAT: an unknown sample format, bit_width
 * outside 1..8 (int8) or 1..16 (int16; ignored for cf32).  Per call PFB_ERR_BAD_ARG: a null handle, an unknown mem,
 * ld != 1 for an integer format or ld = 0, num_pulses > 2^24, num_samples ld overflowing 2^63 elements, null x with
 * num_samples > 0, null pulses or rec_out with num_pulses > 0, a device pointer not aligned (one element for x, 8
 * bytes for pulses and records, 4 for negs_out).  negs_out == NULL with max_negatives > 0 is allowed: no list is
 * written.  Then PFB_ERR_NO_DEVICE without a HIP device. */
enum {
  PFB_MOP_OUTSIDE = 1,
  PFB_MOP_SHORT = 2,
  PFB_MOP_TRUNCATED = 4,
  PFB_MOP_NEGS_CLIPPED = 8
};
enum { /* pfb_mop_figure.kind */
  PFB_MOP_KIND_UNMODULATED = 0,
  PFB_MOP_KIND_LFM = 1,
  PFB_MOP_KIND_PHASE_CODED = 2,
  PFB_MOP_KIND_BOTH = 3,
  PFB_MOP_KIND_NOT_MEASURABLE = 4
};

typedef struct pfb_mop_config {
  uint32_t struct_size;    /* = sizeof(pfb_mop_config)                         */
  uint32_t sample_format;  /* PFB_FMT_*                                        */
  uint32_t bit_width;      /* of the integer formats; the sums are in counts   */
  uint32_t trim_samples;   /* t: samples left out at each end, <= 2^19         */
  uint32_t max_negatives;  /* entries per pulse of negs_out, 0 .. 128          */
  int32_t device_id;       /* -1 = the current device                          */
} pfb_mop_config;

typedef struct pfb_mop_pulse { /* 16 bytes */
  uint64_t start;          /* global index of the first sample                 */
  uint32_t length;         /* samples                                          */
  uint32_t column;         /* cf32 with a pitch: the column; else 0            */
} pfb_mop_pulse;

typedef struct pfb_mop_record { /* 96 bytes */
  uint64_t start;          /* echoed                                           */
  uint32_t length;
  uint32_t column;
  uint32_t n;              /* samples measured                                 */
  uint32_t flags;          /* PFB_MOP_*                                        */
  uint32_t neg_count;
  uint32_t first_neg;
  uint32_t last_neg;
  uint32_t peak_index;
  uint32_t negs_listed;
  uint32_t reserved;       /* 0 */
  double energy;
  double peak_power;
  double s1_re, s1_im;
  double s2_re, s2_im;
} pfb_mop_record;

typedef struct pfb_mop_plan { /* what pfb_mop_describe reports; host only */
  uint64_t scratch_bytes;  /* device memory a handle holds after a device-route call on a list of any length */
  uint32_t group_min;      /* the least n that mop_group takes                 */
  uint32_t split_min;      /* the least n that mop_split takes                 */
  uint32_t part_samples;   /* i per part of a split pulse                      */
  uint32_t grid_cap;       /* workgroups of a launch at most                   */
  uint32_t threads;        /* lanes of a workgroup                             */
  uint32_t slice_pulses;   /* pulses one round of launches takes               */
  uint32_t split_slots;    /* split pulses one mop_split launch takes          */
  uint32_t stage_bytes;    /* the host route's staging chunk                   */
  char wave_kernel[32];
  char group_kernel[32];
  char split_kernel[32];
  char join_kernel[32];
} pfb_mop_plan;

typedef struct pfb_mop_figure { /* 48 bytes; what pfb_mop_figures makes of a record */
  double freq_hz;          /* atan2(s1_im, s1_re) / (2 pi) fs                  */
  double rate_hz_per_s;    /* atan2(s2_im, s2_re) / (2 pi L) fs^2; 0 when L = 0 */
  double extent_hz;        /* rate (n - 1) / fs                                */
  double mean_power;       /* energy / n; 0 when n = 0                         */
  double flips;            /* neg_count / 2                                    */
  uint32_t kind;           /* PFB_MOP_KIND_*                                   */
  uint32_t reserved;       /* 0 */
} pfb_mop_figure;

typedef struct pfb_mop_handle pfb_mop_handle;

/* Host only: validate cfg (everything pfb_mop_create checks before the device) and report the plan. */
int pfb_mop_describe(const pfb_mop_config* cfg, pfb_mop_plan* plan_out);
/* Lifecycle as pfb_deint_*.  The scratch is of a fixed size; the host route's staging grows to the longest window. */
int pfb_mop_create(const pfb_mop_config* cfg, pfb_mop_handle** out);
int pfb_mop_destroy(pfb_mop_handle* h);
int pfb_mop_set_stream(pfb_mop_handle* h, void* hip_stream);
int pfb_mop_sync(pfb_mop_handle* h);
int pfb_mop_get_device(const pfb_mop_handle* h, int* device_id);
/* Measure num_pulses pulses of x.  x is host or device memory by mem, the pulse list independently by pulses_mem;
 * rec_out (num_pulses records) and negs_out (num_pulses max_negatives uint32, or NULL) follow pulses_mem.
 * Synchronous. */
int pfb_mop_measure(pfb_mop_handle* h, const void* x, uint64_t num_samples, uint64_t ld, uint64_t base_index, uint32_t mem,
                    const pfb_mop_pulse* pulses, uint64_t num_pulses, uint32_t pulses_mem, pfb_mop_record* rec_out,
                    uint32_t* negs_out);
/* The same with every pointer in device memory: launches on the handle's stream and does not wait for it. */
int pfb_mop_measure_async(pfb_mop_handle* h, const void* x, uint64_t num_samples, uint64_t ld, uint64_t base_index,
                          const pfb_mop_pulse* pulses, uint64_t num_pulses, pfb_mop_record* rec_out, uint32_t* negs_out);
/* The kernels the last call launched, joined with '+'; "" before the first and after a call that launched none. */
const char* pfb_mop_last_kernel(const pfb_mop_handle* h);
/* Host only: records into physical figures at sample rate fs, in double.  kind: NOT_MEASURABLE when n < 3 or OUTSIDE;
 * else bit 0 (LFM) when |extent_hz| >= fs / n, one Rayleigh bin of the pulse, and bit 1 (phase coded) when
 * neg_count >= 2.  PFB_ERR_BAD_ARG for null pointers with n > 0 or an fs that is not finite or <= 0. */
int pfb_mop_figures(const pfb_mop_record* records, uint64_t n, double fs, pfb_mop_figure* out);
/* Host only: pulses from PDWs whose toa and pw are in seconds of a series at series_rate rows a second that began at
 * t0: start = llrint((toa - t0) series_rate) - 1 (the scripts' toa is 1-based), length = llrint(pw series_rate),
 * column = bin.  PFB_ERR_BAD_ARG for null pointers with n > 0, n > 2^31, a series_rate that is not finite or <= 0, a
 * t0, toa or pw that is not finite, a start under 0 or at or over 2^62, a length under 0 or over 2^32 - 1, a negative
 * bin; nothing is written then. */
int pfb_mop_pulses_from_pdw(const pfb_pdw* pdws, uint64_t n, double series_rate, double t0, pfb_mop_pulse* pulses_out);

/* ---- Fractional-PRI search and regridder: trains whose period is not a whole number of samples ----
 * pfb_fold_* folds at integer periods and pfb_pd_* integrates at an integer PRI.  An emitter's clock is not locked to
 * the recorder's: off the air a PRI is 2048.37 samples, the train drifts a cell every three periods, an integer fold
 * smears it over many bins and a coherent integration walks it through the gates.  This section is the two missing
 * pieces.  pfb_qfold_* is pfb_fold_* at periods given in 2^-32 samples; pfb_regrid_* lays the windows of such a train
 * onto an integer grid, so that pfb_pd_*, pfb_cfar_*, pfb_rdcfar_* and pfb_oscfar_* take it as they are.  This comment
 * is the definition: the device code (csrc/pfb_qfold.hip) and the tests' restatement (tests/qfold_ref.py) are each
 * written from it.
 *
 * Period: Pq, a uint64 holding the period times 2^32; Pi = Pq >> 32, Pf = Pq & (2^32 - 1).  Legal (pfb_qfold_*, with
 * bin_cells C): C <= Pi <= 2^24 and NB = floor(Pi / C) <= 65536 bins.  Period m begins at cell
 *   start(m) = ceil(m Pq / 2^32) = m Pi + ceil(m Pf / 2^32),
 * so every period is Pi or Pi + 1 cells long and start is strictly increasing.  The period of global cell i is
 * m(i) = floor(i 2^32 / Pq), the largest m with start(m) <= i.
 *
 * Bin of cell i:  j = min(floor((i - start(m(i))) / C), NB - 1).  Every bin of a period but the last is exactly C
 * cells; the last takes what is left, Pi - (NB - 1) C cells or one more in a long period.  With Pf = 0 this is
 * pfb_fold_*'s rule word for word.
 *
 * Profile, invariance and limits are pfb_fold_*'s: F[j] is the float32 sum of the cells of bin j, added ONE AT A TIME
 * IN ASCENDING i starting from +0.0f, no tree, no atomics, no partial sums combined later; the same bits come out under
 * any cutting of the stream into calls, empty calls included; NaN and Inf go where IEEE addition takes them.  1 <= NC <=
 * 4096 candidates, C = 1 .. 64, duplicates allowed, profiles of sum_c NB_c * 4 bytes <= 64 MiB (PFB_ERR_UNSUPPORTED
 * above), stream index <= 2^62.
 *
 * Start index: pfb_qfold_set_index(h, N0) clears the profiles and makes N0 (<= 2^62) the index of the next cell.  Cells
 * before N0 count as never seen.  A caller skips the head of a record with it.  pfb_qfold_reset is set_index(0).
 *
 * Counts, all integers.  With n_j(N) the cells i < N of bin j, the handle's count of bin j is n_j(N) - n_j(N0), where,
 * with M = m(N - 1) + 1 the periods begun,
 *   n_j(N) = (M - 1) C + clamp(N - start(M - 1) - j C, 0, C)     for j < NB - 1,
 *   n_{NB-1}(N) = N - sum_{j < NB-1} n_j(N),                       n_j(0) = 0.
 * pfb_qfold_counts (host only, 128-bit host arithmetic) gives n_j(num_cells) - n_j(first_cell).
 *
 * Score: one 64-byte pfb_qfold_score per candidate, in list order.  bins_used counts the bins with a count > 0; after a
 * set_index into the middle of a period these need not be the leading ones.  The means m_j = (double)F[j] / (double)
 * count_j, the peak walk and the two sums run over exactly those bins, j ascending.  The peak walk is pfb_fold_score's:
 * strictly greater replaces, ties go to the lowest j, a NaN never displaces anything, a NaN in the first used bin stays.
 * peak_sum = F[peak_bin], peak_cells its count, peak_mean = (float)m_peak.  sum_means and sum_sq_means have no fixed
 * order and are good to (bins_used + 1) 2^-53 sum |terms|, the bound pfb_fold_* states.  Every other field is a fixed
 * function of the cells.  With no cell taken every field but period_q32, num_bins and cells is 0.  The statistic
 * pfb_fold_* describes (z from peak_mean, sum_means, sum_sq_means, bins_used) applies unchanged; origin = peak_bin C.
 *
 * Regrid (pfb_regrid_*).  Parameters: period_q32 (1 <= Pi <= 2^24), origin o (<= 2^62), row_samples R (1 .. Pi),
 * elem_bytes (8: complex64, 4: float32).  Output element t = k R + r (r < R) is input element o + start(k) + r, copied
 * bit for bit.  The source index rises strictly with t, so a call that takes input [s, s + n) writes one contiguous
 * range of t -- those whose source lies in it -- to out[0 ..).  Their number is known on the host from lengths alone
 * (pfb_regrid_outputs_for): there is no carry and no flush, and any cutting gives the same bytes because nothing is
 * computed.  PFB_ERR_CAPACITY reports the count needed and changes no state.  Pulse k of a train at period Pq that
 * begins at o then sits at k R of the output, so pfb_pd_config{pri = R, origin = 0} takes it; row d of those maps stands
 * for d fs 2^32 / (ND Pq) -- the true period, not R (pfb_regrid_doppler_frequencies, host only).
 *
 * Not built: sub-sample interpolation (a pulse is taken at the first whole sample at or after its true start, up to one
 * sample late), staggered periods.
 *
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers (the list
 * included), a wrong struct_size, C outside 1 .. 64, NC outside 1 .. 4096, a period with Pi < C or Pq > 2^24 2^32 or
 * more than 65536 bins, flags != 0; for pfb_regrid_* a period with Pi < 1 or Pq > 2^24 2^32, an origin > 2^62, R outside
 * 1 .. Pi, elem_bytes not 4 or 8, flags != 0; per call an unknown mem, a device pointer not aligned to its element (4
 * bytes for cells and profiles, 8 for score records and counts, elem_bytes for regrid elements), an index that would
 * pass 2^62, a candidate >= NC.  Then PFB_ERR_UNSUPPORTED: profiles over 64 MiB.  Then PFB_ERR_NO_DEVICE without a HIP
 * device.  Then, per call, PFB_ERR_CAPACITY. */
typedef struct pfb_qfold_config {
  uint32_t struct_size;       /* = sizeof(pfb_qfold_config)                                      */
  uint32_t bin_cells;         /* C                                                               */
  uint32_t num_periods;       /* NC                                                              */
  uint32_t flags;             /* 0                                                               */
  const uint64_t* periods_q32;/* Pq_c, c = 0 .. NC-1, copied at create                           */
  int32_t device_id;          /* HIP device ordinal, -1 = current device                         */
  uint32_t reserved;          /* ignored                                                         */
} pfb_qfold_config;

typedef struct pfb_qfold_plan { /* what pfb_qfold_describe reports; host only                    */
  uint64_t profile_bytes;     /* sum_c NB_c * 4 (the handle holds a second copy: pfb_qfold_process) */
  uint64_t total_bins;        /* sum_c NB_c                                                      */
  uint32_t max_bins;          /* max_c NB_c                                                      */
  char kernel[32];            /* the kernel that folds a call                                    */
} pfb_qfold_plan;

typedef struct pfb_qfold_score {  /* 64 bytes */
  uint64_t period_q32;           /* Pq                                                               */
  uint32_t num_bins, bins_used;  /* NB; bins with a count > 0                                        */
  uint32_t peak_bin, reserved;   /* the used bin of largest mean, ties to the lowest; 0              */
  uint64_t peak_cells;           /* its count                                                        */
  float peak_sum, peak_mean;     /* F[peak_bin]; (float)m_peak                                       */
  double sum_means, sum_sq_means;
  uint64_t cells;                /* N - N0 */
} pfb_qfold_score;

typedef struct pfb_qfold_handle pfb_qfold_handle;

/* Host only: validate cfg (everything pfb_qfold_create checks before the device) and report the plan. */
int pfb_qfold_describe(const pfb_qfold_config* cfg, pfb_qfold_plan* plan_out);
/* Host only: counts_out[j] = n_j(num_cells) - n_j(first_cell) for the NB bins of candidate `candidate` of cfg.
 * PFB_ERR_BAD_ARG for a cfg pfb_qfold_describe refuses with it, a null counts_out, candidate >= NC, first_cell >
 * num_cells, num_cells > 2^62. */
int pfb_qfold_counts(const pfb_qfold_config* cfg, uint32_t candidate, uint64_t first_cell, uint64_t num_cells,
                     uint64_t* counts_out);
/* Lifecycle as pfb_fold_*.  The handle owns the period list, the profiles and, per candidate, where in its period the
 * next cell lies. */
int pfb_qfold_create(const pfb_qfold_config* cfg, pfb_qfold_handle** out);
int pfb_qfold_destroy(pfb_qfold_handle* h);
int pfb_qfold_reset(pfb_qfold_handle* h);   /* pfb_qfold_set_index(h, 0) */
int pfb_qfold_set_index(pfb_qfold_handle* h, uint64_t next_cell);  /* profiles to +0, N0 = N = next_cell; waits for the stream */
int pfb_qfold_set_stream(pfb_qfold_handle* h, void* hip_stream);
int pfb_qfold_sync(pfb_qfold_handle* h);
int pfb_qfold_get_device(const pfb_qfold_handle* h, int* device_id);
int pfb_qfold_next_index(const pfb_qfold_handle* h, uint64_t* index_out);  /* N: global index of the next cell taken */
/* Fold num_cells cells into every profile: memory contracts, staging and what PFB_ERR_HIP leaves behind exactly as
 * pfb_fold_process states them.  Synchronous. */
int pfb_qfold_process(pfb_qfold_handle* h, const float* cells, uint64_t num_cells, uint32_t mem);
/* Same, device pointer, enqueued on the handle's stream without a host sync. */
int pfb_qfold_process_async(pfb_qfold_handle* h, const float* d_cells, uint64_t num_cells);
/* The NC score records of the cells taken so far, as pfb_fold_scores: PFB_ERR_CAPACITY when capacity < NC. */
int pfb_qfold_scores(pfb_qfold_handle* h, pfb_qfold_score* out, uint64_t capacity, uint32_t mem);
/* F of one candidate, NB floats, as pfb_fold_profile. */
int pfb_qfold_profile(pfb_qfold_handle* h, uint32_t candidate, float* out, uint64_t capacity_bins, uint32_t mem);
/* The kernel the last call that took cells launched: plan.kernel; "" before the first. */
const char* pfb_qfold_last_kernel(const pfb_qfold_handle* h);

typedef struct pfb_regrid_config {
  uint32_t struct_size;       /* = sizeof(pfb_regrid_config)                                     */
  uint32_t row_samples;       /* R, 1 .. Pi                                                      */
  uint64_t period_q32;        /* Pq                                                              */
  uint64_t origin;            /* o: input index of row 0's first element                         */
  uint32_t elem_bytes;        /* 8 (complex64) or 4 (float32)                                    */
  uint32_t flags;             /* 0                                                               */
  int32_t device_id;          /* HIP device ordinal, -1 = current device                         */
  uint32_t reserved;          /* ignored                                                         */
} pfb_regrid_config;

typedef struct pfb_regrid_handle pfb_regrid_handle;

int pfb_regrid_create(const pfb_regrid_config* cfg, pfb_regrid_handle** out);
int pfb_regrid_destroy(pfb_regrid_handle* h);
int pfb_regrid_reset(pfb_regrid_handle* h);   /* input index back to 0 */
int pfb_regrid_set_index(pfb_regrid_handle* h, uint64_t next_input);  /* <= 2^62: the index of the next input element */
int pfb_regrid_set_stream(pfb_regrid_handle* h, void* hip_stream);
int pfb_regrid_sync(pfb_regrid_handle* h);
int pfb_regrid_get_device(const pfb_regrid_handle* h, int* device_id);
int pfb_regrid_next_index(const pfb_regrid_handle* h, uint64_t* index_out);
/* The output elements the next num_inputs input elements give, from the handle's index and lengths alone. */
int pfb_regrid_outputs_for(const pfb_regrid_handle* h, uint64_t num_inputs, uint64_t* outputs_out);
/* Take num_inputs elements; the output elements whose source lies among them go to out[0 ..) (room for
 * capacity_outputs), their number to *outputs_out.  PFB_ERR_CAPACITY sets *outputs_out to the number needed and changes
 * no state.  mem: x and out are both host pointers (staged through the device) or both device pointers.  Synchronous. */
int pfb_regrid_process(pfb_regrid_handle* h, const void* x, uint64_t num_inputs, void* out, uint64_t capacity_outputs,
                       uint64_t* outputs_out, uint32_t mem);
/* Same, device pointers, enqueued on the handle's stream without a host sync; the count is written to *d_outputs_out,
 * a uint64 in device memory, in stream order.  PFB_ERR_CAPACITY queues nothing. */
int pfb_regrid_process_async(pfb_regrid_handle* h, const void* d_x, uint64_t num_inputs, void* d_out,
                             uint64_t capacity_outputs, uint64_t* d_outputs_out);
/* Host only: out[i] = d fs 2^32 / (ND Pq) for the ND = doppler_length rows in the order pfb_pd_* writes them (d = 0 ..
 * ND-1, or -ND/2 .. ND/2-1 with centered != 0).  PFB_ERR_BAD_ARG for a null out, a period pfb_regrid_create refuses, ND
 * outside 1 .. 65536 or fs not finite. */
int pfb_regrid_doppler_frequencies(uint64_t period_q32, uint32_t doppler_length, int centered, double fs, double* out);

/* ---- PDW association: one record per pulse across channels ---------------------------------------
 * The channelized extractor (pfb_pdw_extract) runs one edge state machine per channel and returns one PDW per
 * (channel, pulse).  A pulse is never in one channel only: a chirp walks through the channels, a carrier near a channel
 * edge sits in two, and every pulse edge is wideband and leaves one-frame rows in the neighbouring columns.  This unit
 * joins the rows of one pulse: rows that touch in time and lie in neighbouring cells are linked, and a connected set
 * of rows is one group with one record.  It is the piece that the deinterleaver's section lists as not built
 * (clustering before the time search): pfb_deint_* takes the groups' first_tick.  Every figure is an integer or a
 * comparison, so the results are bytes, not tolerances.  This comment is the definition: the device code
 * (csrc/pfb_assoc.hip) and the tests' restatement (tests/assoc_ref.py) are each written from it.
 *
 * Input: N <= 2^20 items pfb_assoc_item (24 bytes) in host or device memory by `mem` (a device pointer is 8-byte
 * aligned): start and length in the caller's ticks, cell (a PDW's bin), weight (a PDW's mag).  start is non-decreasing;
 * the order among equal starts is the caller's.  With end = start + length, every end + g is below 2^62.  `reserved`
 * is written as 0 and is not read.
 *
 * Parameters: Rc = cell_reach (0 .. 64), g = slack_ticks (0 .. 2^31 - 1), K = window_items (1 .. 4096), flags = 0.
 *
 * Edge.  Items i < j are linked iff j - i <= K, start[j] <= end[i] + g and |cell[i] - cell[j]| <= Rc.  start[j] >=
 * start[i] by the order, which is the other half of the overlap test.  The search of item i ends at the first j with
 * start[j] > end[i] + g, or at j = i + K.  Item i is CLIPPED iff i + K + 1 < N and start[i + K + 1] <= end[i] + g: the
 * window ended the search, not the time.
 *
 * Groups.  A group is a connected component of that graph; its root is its smallest index; groups are numbered by
 * ascending root.  labels[i] (int32) is the group of item i: every item has one, a lone item is a group of one.
 *
 * Record, pfb_assoc_group: first_tick = the root's start, end_tick = the largest end, length_sum, members, first_item =
 * the root, best_item = the member with the largest weight, best_cell = its cell, cell_lo / cell_hi = the smallest and
 * largest cell.  The order of the weights is that of the order-preserving uint32 key of the float's bits (all bits of
 * a negative flipped, the sign bit of the rest flipped: -NaN < -Inf < -0 < +0 < +Inf < +NaN); ties go to the lowest index.
 *
 * Stats of the last good run: groups, edges (pairs that satisfy the rule), clipped, largest_group (members),
 * linked_items (items in groups of two or more), rounds.  `rounds` is how often the device went round (below); it is
 * reported, but it is not a function of the input alone and is never compared.  Everything else is a pure function of
 * the list and the config: THE SAME CALL TWICE, AND HOST AND DEVICE INPUT, GIVE THE SAME BYTES.
 *
 * Device.  A first pass splits the items into arrays, checks the order and the bound and labels every item with its
 * own index.  Edge pass: one lane per item walks the item's window; for K <= 1024 (pfb_assoc_plan.lds_window) a
 * workgroup of 256 items (tile_items) first stages the start and cell of its items and of the K + 1 behind them, and
 * its own end + g, in LDS as separate arrays (pfb_assoc_link_lds); above that, or by pfb_assoc_set_tier, it reads the
 * window through the caches (pfb_assoc_link_global).  Components: rounds of hooking (for every edge whose two labels
 * differ, an integer atomic min on the larger label's entry with the smaller; pfb_assoc_hook) and ceil(log2 N) + 1
 * passes of pointer doubling (pfb_assoc_jump), until a round hooks nothing; the host reads one flag a round and gives
 * up with PFB_ERR_INTERNAL after 64.  A label only decreases and never exceeds its index, so the fixed point is the
 * smallest index of each component whatever the timing.  Records: root flags, a scan and an ordered scatter number the
 * groups (pfb_assoc_number), integer min / max / add atomics and one 64-bit max of (key << 32 | ~index) fill them
 * (pfb_assoc_gather).  There are no float atomics.  pfb_assoc_last_kernel joins the names of what the last call launched
 * with '+'.
 *
 * Not built: a device sort (items arrive sorted; pfb_assoc_items_from_pdws sorts on the host), an async form (a
 * round's decision returns to the host), a streaming form over chunks of a list, clustering on measured frequency or
 * pulse width instead of the cell (that is pfb_cluster_*), weighted centroids (float sums: the host can form them from the labels).
 *
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers, a wrong
 * struct_size, cell_reach > 64, slack_ticks > 2^31 - 1, window_items outside 1 .. 4096, flags != 0; per call a null
 * handle, an unknown mem, n > 2^20, a null items with n > 0, a null output (groups_out may be null only with capacity
 * = 0, labels_out and the link arrays only with n = 0), a device pointer not aligned to its element (8 bytes for items
 * and records, 4 for labels and the link arrays).  Then PFB_ERR_NO_DEVICE without a HIP device.  The order of the
 * starts and the bound 2^62 are checked on the device, in the first pass over the list: a list that fails returns
 * PFB_ERR_BAD_ARG with nothing written. */
typedef struct pfb_assoc_item {   /* 24 bytes */
  uint64_t start;             /* ticks                                                            */
  uint32_t length;            /* ticks; end = start + length                                      */
  int32_t cell;               /* the channel, or any integer coordinate                           */
  float weight;               /* what picks the best member                                       */
  uint32_t reserved;          /* 0                                                                */
} pfb_assoc_item;

typedef struct pfb_assoc_config {
  uint32_t struct_size;       /* = sizeof(pfb_assoc_config)                                       */
  uint32_t cell_reach;        /* Rc                                                               */
  uint32_t slack_ticks;       /* g                                                                */
  uint32_t window_items;      /* K: how far behind an item its links are looked for               */
  uint32_t flags;             /* 0                                                                */
  int32_t device_id;          /* -1 = the current device                                          */
} pfb_assoc_config;

typedef struct pfb_assoc_plan {  /* what pfb_assoc_describe reports; host only                    */
  uint64_t scratch_bytes;     /* device memory a handle holds after pfb_assoc_run on n items      */
  uint32_t tile_items;        /* items of one workgroup of the edge pass                          */
  uint32_t lds_window;        /* the largest K the LDS tier takes                                 */
  uint32_t lds_bytes;         /* of one workgroup of the edge pass at this K                      */
  uint32_t reserved;          /* 0 */
  char link_kernel[32];
  char component_kernel[32];
  char record_kernel[32];
} pfb_assoc_plan;

typedef struct pfb_assoc_group {  /* 48 bytes */
  uint64_t first_tick;        /* the root's start                                                 */
  uint64_t end_tick;          /* the largest end                                                  */
  uint64_t length_sum;        /* of the members' lengths                                          */
  uint32_t members;
  uint32_t first_item;        /* the root: the group's smallest index                             */
  uint32_t best_item;         /* the member of largest weight, ties to the lowest index           */
  int32_t best_cell;          /* its cell                                                         */
  int32_t cell_lo;            /* the smallest cell                                                */
  int32_t cell_hi;            /* the largest                                                      */
} pfb_assoc_group;

typedef struct pfb_assoc_stats {
  uint64_t groups;
  uint64_t edges;
  uint64_t clipped;
  uint64_t largest_group;
  uint64_t linked_items;
  uint64_t rounds;            /* not a function of the input alone                                */
} pfb_assoc_stats;

typedef struct pfb_assoc_handle pfb_assoc_handle;

/* Host only: validate cfg (everything pfb_assoc_create checks before the device) and report the plan for a list of
 * n items (n > 2^20: PFB_ERR_BAD_ARG). */
int pfb_assoc_describe(const pfb_assoc_config* cfg, uint64_t n, pfb_assoc_plan* plan_out);
/* Lifecycle as pfb_deint_*.  The scratch grows with the longest list seen and is kept. */
int pfb_assoc_create(const pfb_assoc_config* cfg, pfb_assoc_handle** out);
int pfb_assoc_destroy(pfb_assoc_handle* h);
int pfb_assoc_set_stream(pfb_assoc_handle* h, void* hip_stream);
int pfb_assoc_sync(pfb_assoc_handle* h);
int pfb_assoc_get_device(const pfb_assoc_handle* h, int* device_id);
/* The whole association.  groups_out (capacity records) and labels_out (n int32) are host memory, or device memory
 * with mem = PFB_MEM_DEVICE; *count_out (host) is the number of groups.  PFB_ERR_CAPACITY when that is more than
 * capacity: *count_out holds the true count, neither array is written and the stats stay those of the run before.
 * Synchronous. */
int pfb_assoc_run(pfb_assoc_handle* h, const pfb_assoc_item* items, uint64_t n, uint32_t mem, pfb_assoc_group* groups_out,
                  uint64_t capacity, uint64_t* count_out, int32_t* labels_out);
/* The edge search alone: per item the lowest linked j > i (-1 for none) and the number of linked j > i, n int32 each.
 * Changes no stats. */
int pfb_assoc_links(pfb_assoc_handle* h, const pfb_assoc_item* items, uint64_t n, uint32_t mem, int32_t* first_link_out,
                    int32_t* link_count_out);
/* The kernels the last call launched, joined with '+'; "" before the first and after a call that launched none. */
const char* pfb_assoc_last_kernel(const pfb_assoc_handle* h);
/* The stats of the last pfb_assoc_run that returned PFB_OK; zeros before the first. */
int pfb_assoc_get_stats(const pfb_assoc_handle* h, pfb_assoc_stats* stats_out);
/* Host only: items from a PDW table in any order.  start = llrint((toa - t0) tick_rate), length = llrint(pw
 * tick_rate), cell = bin, weight = (float)mag, sorted by start ascending and stably: items_out[i] comes from
 * pdws[order_out[i]].  PFB_ERR_BAD_ARG as pfb_deint_ticks_from_toa: null pointers, n > 2^31, a tick_rate that is not
 * finite or <= 0, a t0 that is not finite, a toa or pw that is not finite, a negative start or one >= 2^62, a length
 * that is negative or >= 2^32; nothing is written then. */
int pfb_assoc_items_from_pdws(const pfb_pdw* pdws, uint64_t n, double t0, double tick_rate, pfb_assoc_item* items_out,
                              uint32_t* order_out);

/* ---- PDW clustering: cells of frequency and pulse width before the time search -------------------
 * The deinterleaver (pfb_deint_*) searches ONE time-ordered list for periods; with tens of trains in it thousands of
 * histogram bins pass the candidate rule and nearly all are refused.  Emitters differ in frequency and pulse width
 * long before they differ in period, so the first stage of a deinterleaver is a cell clustering on those two: this
 * unit.  It takes two integer features per pulse, counts the pulses of every cell of a U x V grid, joins the dense
 * cells that lie near each other into clusters, and returns per pulse its cluster and per cluster the pulses' indices
 * in the caller's (time) order, ready to be cut out of the tick list (pfb_cluster_gather) and searched one cluster at
 * a time.  Every figure is an integer or a comparison, so the results are bytes, not tolerances.  This comment is the
 * definition: the device code (csrc/pfb_cluster.hip) and the tests' restatement (tests/cluster_ref.py) are each
 * written from it.
 *
 * Input: N <= 2^20 items pfb_cluster_item {int32 u; int32 v;} (8 bytes) in host or device memory by `mem` (a device
 * pointer is 8-byte aligned), in the caller's order: the time order the deinterleaver wants.  Any int32 is a valid u
 * or v.
 *
 * Parameters: U = cells_u, V = cells_v (each >= 1, U V <= 2^20), reach_u, reach_v (0 .. 8), min_cell_count
 * (1 .. 2^20), min_pulses (1 .. 2^20), flags (0 or PFB_CLUSTER_BORDER).
 *
 * An item is IN THE GRID iff 0 <= u < U and 0 <= v < V; its cell is g = u V + v, and cell g has u = g / V, v = g mod V.
 *  1. Histogram: H[g], uint32, is the number of in-grid items of cell g.  A count of a set: the order is free.
 *  2. Dense: cell g is dense iff H[g] >= min_cell_count.
 *  3. Components: dense cells (u, v) and (u', v') are linked iff |u - u'| <= reach_u and |v - v'| <= reach_v.  A
 *     component is a connected set of dense cells; its root is its lowest g.
 *  4. Border, only with PFB_CLUSTER_BORDER: a cell with 0 < H[g] < min_cell_count whose reach box (the cells within
 *     reach_u and reach_v of it) holds at least one dense cell joins the component of the LOWEST ROOT among the dense
 *     cells of its box.  It links nothing onwards: two components that share a border cell stay two.  Without the
 *     flag such cells belong to nobody.
 *  5. Clusters: pulses(component) = the sum of H over its dense and border cells.  A component is a cluster iff
 *     pulses >= min_pulses.  Clusters are numbered 0 .. G - 1 by ascending root.  G <= 65535: a call that finds more,
 *     or more than its `capacity`, returns PFB_ERR_CAPACITY with *count_out = G, writes nothing else and leaves the
 *     stats those of the run before.
 *  6. Output.  labels[i], int32: the cluster of item i, or -1 (outside the grid, in a cell of no component, or in a
 *     component under min_pulses).  One pfb_cluster_group per cluster: root_u, root_v; pulses; cells (dense and
 *     border); u_min .. v_max over its cells; sum_u, sum_v over its items (the host forms centroids, as for
 *     pfb_assoc_*); peak_u, peak_v, peak_count: the cell of largest H, ties to the lowest g; first_item, the lowest
 *     item index.  order_out[N], uint32: the item indices sorted by (label with -1 last, index) -- a STABLE partition,
 *     time order is kept within a cluster.  offsets_out[G + 2], uint32: cluster c's items are order[offsets[c] ..
 *     offsets[c + 1]), the unassigned are order[offsets[G] .. offsets[G + 1]) and offsets[G + 1] = N.  order_out and
 *     offsets_out may be null together.
 * Everything is a pure function of the list and the config: THE SAME CALL TWICE, AND HOST AND DEVICE INPUT, GIVE THE
 * SAME BYTES.
 *
 * Stats of the last good run: outside (items not in the grid), unassigned (in-grid items with label -1), dense_cells,
 * border_cells (cells that step 4 joined), components (before min_pulses), hook_rounds.  hook_rounds is defined by
 * the rounds of step 3 as the device makes them, and is a function of the input too.  Every dense cell starts with
 * the label L[g] = g.  One round: with L as it stands, every linked pair of dense cells whose labels a = L[g] < b =
 * L[g'] differ lowers the new label of cell b to at most a (all pairs read the same L; the new labels start as L);
 * then every cell's label is replaced by the label at the end of its chain g -> L[g] -> ... .  hook_rounds counts the
 * rounds made, the last of which lowered nothing; it is 0 when no cell is dense.
 *
 * Device.  Histogram: one lane per item, pfb_cluster_plan.hist_tile items a workgroup; for U V <= 8192
 * (pfb_cluster_plan.lds_cells) a workgroup counts in a private LDS histogram that it adds to the global one once
 * (pfb_cluster_hist_lds), above that straight into the global one (pfb_cluster_hist_global).  In both a wave first
 * combines the lanes that hit the same cell as its first remaining lane, twice, so that a train that sits in one cell
 * costs one atomic a wave.  Components: one lane per cell, a workgroup takes a block of block_u x block_v cells and
 * stages their labels with a halo of the reach in LDS (pfb_cluster_hook); a lowered label is an integer atomic min
 * into the new labels; ceil(log2 U V) + 1 passes of pointer doubling follow (pfb_cluster_jump); the host reads one
 * flag a round and gives up with PFB_ERR_INTERNAL after 64.  Border: one lane per cell, a min over the box
 * (pfb_cluster_border).  Per-root integer add / min / max atomics and one 64-bit max of (H << 32 | ~g) collect what a
 * record takes from the cells (pfb_cluster_cells); root flags, a scan and an ordered scatter number the clusters
 * (pfb_cluster_number).  Labels: one lane per item, label_tile items a workgroup, a gather through the cell table and
 * wave-combined 64-bit adds and a min for sum_u, sum_v and first_item (pfb_cluster_label).  Partition: an LSD radix
 * over the label (-1 taken as G) with 8-bit digits, one pass when G + 1 <= 256 and two above; a pass is a digit
 * histogram per tile of part_tile items, a scan over (digit, tile) and a rank inside the tile made of wave ballots,
 * the count of lower lanes and the counts of lower waves through LDS -- no atomics, so the order never depends on
 * arrival (pfb_cluster_part1 / pfb_cluster_part2).  There is no float on the device.  pfb_cluster_last_kernel joins
 * the names of what the last call launched with '+'.
 *
 * Not built: more than two features, float features on the device, an async form (a round's decision returns to the
 * host), a streaming form over chunks of a list, density-reachability beyond the border rule, the deinterleaver's
 * rounds for all clusters in one launch.
 *
 * Every argument is validated before the device is touched, in this order.  PFB_ERR_BAD_ARG: null pointers, a wrong
 * struct_size, cells_u = 0, cells_v = 0, U V > 2^20, reach_u > 8, reach_v > 8, min_cell_count outside 1 .. 2^20,
 * min_pulses outside 1 .. 2^20, flags with a bit other than PFB_CLUSTER_BORDER; per call a null handle, an unknown
 * mem, n > 2^20, a null items with n > 0, a null output (count_out never; groups_out may be null only with capacity =
 * 0, labels_out only with n = 0; order_out and offsets_out only together), a device pointer not aligned to its
 * element (8 bytes for items and records, 4 for labels, order, offsets, counts and roots); for pfb_cluster_gather an
 * elem_bytes other than 4 or 8, n > 2^20, a null src, order or dst with n > 0, src or dst not aligned to elem_bytes,
 * order not aligned to 4.  PFB_ERR_CAPACITY: capacity_cells < U V.  Then PFB_ERR_NO_DEVICE without a HIP device. */
#define PFB_CLUSTER_BORDER 1u     /* step 4 */

typedef struct pfb_cluster_item {   /* 8 bytes */
  int32_t u;                  /* the first feature's cell: frequency                              */
  int32_t v;                  /* the second: pulse width; 0 where there is one feature            */
} pfb_cluster_item;

typedef struct pfb_cluster_config {
  uint32_t struct_size;       /* = sizeof(pfb_cluster_config)                                     */
  uint32_t cells_u;           /* U                                                                */
  uint32_t cells_v;           /* V                                                                */
  uint32_t reach_u;
  uint32_t reach_v;
  uint32_t min_cell_count;    /* items that make a cell dense                                     */
  uint32_t min_pulses;        /* items that make a component a cluster                            */
  uint32_t flags;             /* 0 or PFB_CLUSTER_BORDER                                          */
  int32_t device_id;          /* -1 = the current device                                          */
} pfb_cluster_config;

typedef struct pfb_cluster_plan {  /* what pfb_cluster_describe reports; host only                */
  uint64_t scratch_bytes;     /* device memory a handle holds after pfb_cluster_run on n items    */
  uint32_t cells;             /* U V                                                              */
  uint32_t lds_cells;         /* the largest U V the LDS histogram takes                          */
  uint32_t hist_tile;         /* items of one workgroup of the histogram                          */
  uint32_t label_tile;        /* of the label kernel                                              */
  uint32_t part_tile;         /* of a partition pass                                              */
  uint32_t block_u;           /* cells of one workgroup of the component kernels, along u         */
  uint32_t block_v;           /* and along v; block_u block_v = 256                               */
  uint32_t lds_bytes;         /* of one histogram workgroup                                       */
  uint32_t max_clusters;      /* 65535                                                            */
  uint32_t reserved;          /* 0 */
  char histogram_kernel[32];
  char component_kernel[32];
  char partition_kernel[32];
} pfb_cluster_plan;

typedef struct pfb_cluster_group {  /* 64 bytes */
  int32_t root_u;             /* the lowest cell of the cluster                                   */
  int32_t root_v;
  uint32_t pulses;            /* items                                                            */
  uint32_t cells;             /* dense and border cells                                           */
  int32_t u_min;              /* over its cells                                                   */
  int32_t u_max;
  int32_t v_min;
  int32_t v_max;
  int64_t sum_u;              /* over its items                                                   */
  int64_t sum_v;
  int32_t peak_u;             /* the cell of largest H, ties to the lowest g                      */
  int32_t peak_v;
  uint32_t peak_count;        /* its H                                                            */
  uint32_t first_item;        /* the lowest item index                                            */
} pfb_cluster_group;

typedef struct pfb_cluster_stats {
  uint64_t outside;
  uint64_t unassigned;
  uint64_t dense_cells;
  uint64_t border_cells;
  uint64_t components;
  uint64_t hook_rounds;
} pfb_cluster_stats;

typedef struct pfb_cluster_handle pfb_cluster_handle;

/* Host only: validate cfg (everything pfb_cluster_create checks before the device) and report the plan for a list of
 * n items (n > 2^20: PFB_ERR_BAD_ARG). */
int pfb_cluster_describe(const pfb_cluster_config* cfg, uint64_t n, pfb_cluster_plan* plan_out);
/* Lifecycle as pfb_assoc_*.  The scratch grows with the longest list seen and is kept. */
int pfb_cluster_create(const pfb_cluster_config* cfg, pfb_cluster_handle** out);
int pfb_cluster_destroy(pfb_cluster_handle* h);
int pfb_cluster_set_stream(pfb_cluster_handle* h, void* hip_stream);
int pfb_cluster_sync(pfb_cluster_handle* h);
int pfb_cluster_get_device(const pfb_cluster_handle* h, int* device_id);
/* Steps 1 to 6.  groups_out (capacity records), labels_out (n int32), order_out (n uint32) and offsets_out (G + 2
 * uint32, so capacity + 2 always hold them) are host memory, or device memory with mem = PFB_MEM_DEVICE; *count_out
 * (host) is G.  PFB_ERR_CAPACITY when G is more than capacity or than 65535: *count_out holds G, no array is written
 * and the stats stay those of the run before.  Synchronous. */
int pfb_cluster_run(pfb_cluster_handle* h, const pfb_cluster_item* items, uint64_t n, uint32_t mem,
                    pfb_cluster_group* groups_out, uint64_t capacity, uint64_t* count_out, int32_t* labels_out,
                    uint32_t* order_out, uint32_t* offsets_out);
/* Step 1 alone: U V uint32 counts.  Changes no stats. */
int pfb_cluster_histogram(pfb_cluster_handle* h, const pfb_cluster_item* items, uint64_t n, uint32_t mem,
                          uint32_t* counts_out, uint64_t capacity_cells);
/* Steps 1 to 4 alone: per cell the root g of its component, int32, -1 for none, U V of them.  Border cells count as
 * members; components under min_pulses are included.  For plots and for the tests.  Changes no stats. */
int pfb_cluster_cell_roots(pfb_cluster_handle* h, const pfb_cluster_item* items, uint64_t n, uint32_t mem,
                           int32_t* roots_out, uint64_t capacity_cells);
/* dst[k] = src[order[k]] for k < n, elements of elem_bytes = 4 or 8, all three in device memory, on the handle's
 * stream; returns without waiting (pfb_cluster_sync waits).  Every order[k] indexes src: with order_out of
 * pfb_cluster_run and the tick list the items came from, dst is the list cut into per-cluster lists, cluster c at
 * dst[offsets[c] .. offsets[c + 1]), each in time order: what pfb_deint_run takes. */
int pfb_cluster_gather(pfb_cluster_handle* h, const void* src, uint32_t elem_bytes, const uint32_t* order, uint64_t n,
                       void* dst);
/* The kernels the last call launched, joined with '+'; "" before the first. */
const char* pfb_cluster_last_kernel(const pfb_cluster_handle* h);
/* The stats of the last pfb_cluster_run that returned PFB_OK; zeros before the first. */
int pfb_cluster_get_stats(const pfb_cluster_handle* h, pfb_cluster_stats* stats_out);
/* Host only: items from a PDW table, in the table's order, n PDWs stride_bytes apart (sizeof(pfb_pdw) for a plain
 * array).  u = floor((freq - freq0) / freq_step); v = pw_step > 0 ? floor(pw / pw_step) : 0.  A figure that is not
 * finite or does not fit an int32 gives the item u = INT32_MIN, v = 0, which is outside every grid.  PFB_ERR_BAD_ARG
 * for null pointers with n > 0, n > 2^31, stride_bytes < sizeof(pfb_pdw) or no multiple of 8, a freq0 that is not
 * finite, a freq_step that is not finite or <= 0, a pw_step that is not finite or < 0; nothing is written then. */
int pfb_cluster_items_from_pdws(const pfb_pdw* pdws, uint64_t n, uint64_t stride_bytes, double freq0, double freq_step,
                                double pw_step, pfb_cluster_item* items_out);

#ifdef __cplusplus
}
#endif
#endif
