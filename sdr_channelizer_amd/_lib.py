"""ctypes binding of libpfb_channelizer.so (the C ABI in include/pfb_channelizer.h).

The library is the product: if it is missing this module raises -- there is no
Python or CPU fallback for the channelizer arithmetic.
"""
from __future__ import annotations

import ctypes as C  # noqa: N811
import os
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libpfb_channelizer.so")

PFB_OK = 0
PFB_ERR_BAD_ARG = -1
PFB_ERR_BAD_FORMAT = -2
PFB_ERR_UNSUPPORTED = -3
PFB_ERR_NO_DEVICE = -4
PFB_ERR_HIP = -5
PFB_ERR_NO_MEMORY = -6
PFB_ERR_CAPACITY = -7
PFB_ERR_INTERNAL = -8
PFB_ERR_COMM = -9
PFB_ABI_VERSION = 2
PFB_FREQ_ORDER_FFT, PFB_FREQ_ORDER_CENTERED = 0, 1

PFB_FMT_INT8_IQ, PFB_FMT_INT16_IQ, PFB_FMT_CF32 = 0, 1, 2
PFB_LAYOUT_FRAME_MAJOR, PFB_LAYOUT_CHANNEL_MAJOR = 0, 1
PFB_FLAG_FFTSHIFT, PFB_FLAG_CONJUGATE_INPUT, PFB_FLAG_DEROTATE, PFB_FLAG_MAGNITUDE = 1, 2, 4, 8
PFB_FLAG_POWER = 16  # with PFB_FLAG_MAGNITUDE: |y|^2 instead of |y|
PFB_MEM_HOST, PFB_MEM_DEVICE = 0, 1
PFB_OPT_KERNEL, PFB_OPT_FRAMES_PER_BLOCK, PFB_OPT_HOST_CHUNK_SAMPLES, PFB_OPT_NONTEMPORAL, PFB_OPT_PROFILE, PFB_OPT_XCD_REMAP = 0, 1, 2, 3, 4, 5
PFB_OPT_SCHEDULE, PFB_OPT_GRID, PFB_OPT_TILE_WAVES, PFB_OPT_EXPERIMENT, PFB_OPT_VARIANT = 6, 7, 8, 9, 10
PFB_OPT_SLAB_FRAMES = 11
PFB_STFT_COMPLEX, PFB_STFT_POWER, PFB_STFT_DB = 0, 1, 2
PFB_STFT_CENTERED, PFB_STFT_TWOSIDED = 0, 1
PFB_STFT_KERNEL_AUTO, PFB_STFT_KERNEL_GENERIC, PFB_STFT_KERNEL_FUSED = 0, 1, 2
PFB_DWELL_STAT_MEAN, PFB_DWELL_STAT_MEDIAN = 0, 1
PFB_DWELL_SKIP_FREQ = 1
PFB_SYNTH_BARKER13, PFB_SYNTH_BARKER_DEGREES, PFB_SYNTH_PHASE_FROM_ZERO, PFB_SYNTH_ROUND_MATLAB = 1, 2, 4, 8
PFB_MF_COMPLEX, PFB_MF_POWER = 0, 1
PFB_MF_NORMALIZE = 1
PFB_MF_ROUTE_AUTO, PFB_MF_ROUTE_FUSED, PFB_MF_ROUTE_PARTITIONED = 0, 1, 2
PFB_WF_COMPLEX, PFB_WF_MAGNITUDE, PFB_WF_POWER = 0, 1, 2
PFB_WF_ROWS, PFB_WF_COLUMNS = 0, 1
PFB_CHSYN_FFTSHIFT, PFB_CHSYN_DEROTATE = 1, 2
PFB_CHSYN_ROUTE_AUTO, PFB_CHSYN_ROUTE_FUSED, PFB_CHSYN_ROUTE_GENERIC = 0, 1, 2
PFB_MFBANK_BEST, PFB_MFBANK_SURFACE = 0, 1
PFB_CFAR_POWER, PFB_CFAR_BANK_CELL = 0, 1
PFB_CFAR_CA, PFB_CFAR_GO, PFB_CFAR_SO = 0, 1, 2
PFB_CFAR_DET_ONE_SIDED = 1
PFB_PD_COMPLEX, PFB_PD_POWER, PFB_PD_BEST, PFB_PD_NONCOHERENT = 0, 1, 2, 3
PFB_PD_CENTERED = 1
PFB_RDCFAR_DET_ONE_SIDED = 1
PFB_MOP_OUTSIDE, PFB_MOP_SHORT, PFB_MOP_TRUNCATED, PFB_MOP_NEGS_CLIPPED = 1, 2, 4, 8
PFB_MOP_KIND_UNMODULATED, PFB_MOP_KIND_LFM, PFB_MOP_KIND_PHASE_CODED, PFB_MOP_KIND_BOTH = 0, 1, 2, 3
PFB_MOP_KIND_NOT_MEASURABLE = 4


class PfbConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("num_channels", C.c_uint32), ("taps_per_channel", C.c_uint32),
        ("decimation", C.c_uint32), ("taps", C.POINTER(C.c_float)), ("sample_format", C.c_uint32),
        ("bit_width", C.c_uint32), ("output_layout", C.c_uint32), ("flags", C.c_uint32),
        ("input_offset", C.c_int32), ("device_id", C.c_int32),
    ]


class PfbStftConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("window_length", C.c_uint32), ("hop", C.c_uint32), ("fft_length", C.c_uint32),
        ("window", C.POINTER(C.c_float)), ("sample_format", C.c_uint32), ("bit_width", C.c_uint32),
        ("output", C.c_uint32), ("freq_order", C.c_uint32), ("scale", C.c_double), ("db_floor", C.c_double),
        ("kernel", C.c_uint32), ("device_id", C.c_int32),
    ]


class PfbIqPacket(C.Structure):
    _fields_ = [
        ("endianness", C.c_uint32), ("linkSpeed", C.c_uint32), ("frequencyHz", C.c_uint64),
        ("bandwidthHz", C.c_uint32), ("sampleRateSps", C.c_uint32), ("rxGainDb", C.c_float),
        ("numSamples", C.c_uint32), ("bitWidth", C.c_uint32), ("spare0", C.c_uint32),
        ("boardName", C.c_char * 16), ("serialNumber", C.c_char * 16), ("fpgaVersion", C.c_char * 16),
        ("fwVersion", C.c_char * 16), ("sampleStartTime", C.c_double),
    ]


class PfbPdw(C.Structure):
    _fields_ = [("toa", C.c_double), ("freq", C.c_double), ("pw", C.c_double), ("snr", C.c_double),
                ("sat", C.c_int32), ("bin", C.c_int32), ("mag", C.c_double)]


class PfbDwellConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("sample_format", C.c_uint32), ("bit_width", C.c_uint32), ("statistic", C.c_uint32),
        ("flags", C.c_uint32), ("mem", C.c_uint32), ("device_id", C.c_int32), ("fs", C.c_double), ("fc", C.c_double),
        ("sample_start_time", C.c_double), ("snr_threshold_db", C.c_double), ("sat_fraction", C.c_double),
    ]


class PfbDwellStats(C.Structure):
    _fields_ = [
        ("num_samples", C.c_uint64), ("saturated_components", C.c_uint64), ("pulses", C.c_uint64),
        ("mean_mag", C.c_double), ("peak_mag", C.c_double), ("peak_component", C.c_double),
        ("noise_floor", C.c_double), ("threshold", C.c_double), ("any_pulse_saturated", C.c_int32),
        ("reserved", C.c_int32),
    ]


class PfbSynthConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("sample_format", C.c_uint32), ("bit_width", C.c_uint32), ("flags", C.c_uint32),
        ("pulse_samples", C.c_uint32), ("period_samples", C.c_uint32), ("seed", C.c_uint32), ("device_id", C.c_int32),
        ("first_pulse", C.c_uint64), ("record_samples", C.c_uint64),
        ("fs", C.c_double), ("f0", C.c_double), ("lfm_extent_hz", C.c_double), ("amplitude", C.c_double),
        ("noise_sigma", C.c_double),
    ]


class PfbSynthParams(C.Structure):
    _fields_ = [("pulse_samples", C.c_uint32), ("chip_samples", C.c_uint32), ("fcw", C.c_uint32),
                ("barker_offset", C.c_uint32), ("dcw", C.c_uint64), ("noise_gain", C.c_int64)]


class PfbTraceConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sample_format", C.c_uint32), ("bit_width", C.c_uint32),
                ("bin_samples", C.c_uint32), ("flags", C.c_uint32), ("device_id", C.c_int32)]


class PfbTraceBin(C.Structure):
    _fields_ = [("peak_sample", C.c_uint64), ("power_min", C.c_double), ("power_max", C.c_double),
                ("power_mean", C.c_double), ("peak_i", C.c_float), ("peak_q", C.c_float), ("count", C.c_uint32),
                ("reserved", C.c_uint32)]


class PfbMfConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("replica_length", C.c_uint32), ("replica", C.POINTER(C.c_float)),
                ("sample_format", C.c_uint32), ("bit_width", C.c_uint32), ("output", C.c_uint32), ("flags", C.c_uint32),
                ("fft_length", C.c_uint32), ("route", C.c_uint32), ("device_id", C.c_int32)]


class PfbMfPlan(C.Structure):
    _fields_ = [("fft_length", C.c_uint32), ("route", C.c_uint32), ("partitions", C.c_uint32),
                ("block_outputs", C.c_uint32), ("workspace_bytes", C.c_uint64)]


class PfbWfConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("bin_rows", C.c_uint32), ("element", C.c_uint32),
                ("layout", C.c_uint32), ("flags", C.c_uint32), ("device_id", C.c_int32)]


class PfbWfCell(C.Structure):
    _fields_ = [("power_max", C.c_float), ("power_mean", C.c_float), ("power_min", C.c_float), ("peak_row", C.c_uint32)]


class PfbChsynConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_channels", C.c_uint32), ("taps_per_channel", C.c_uint32),
                ("decimation", C.c_uint32), ("taps", C.POINTER(C.c_float)), ("scale", C.c_double),
                ("output_format", C.c_uint32), ("bit_width", C.c_uint32), ("layout", C.c_uint32), ("flags", C.c_uint32),
                ("route", C.c_uint32), ("device_id", C.c_int32)]


class PfbChsynPlan(C.Structure):
    _fields_ = [("route", C.c_uint32), ("decimation", C.c_uint32), ("q", C.c_uint32), ("tile_frames", C.c_uint32),
                ("carried_bytes", C.c_uint64), ("workspace_bytes", C.c_uint64)]


class PfbMfbankConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("replica_length", C.c_uint32), ("replica", C.POINTER(C.c_float)),
                ("sample_format", C.c_uint32), ("bit_width", C.c_uint32), ("output", C.c_uint32), ("flags", C.c_uint32),
                ("fft_length", C.c_uint32), ("first_bin", C.c_int32), ("num_hypotheses", C.c_uint32),
                ("bin_step", C.c_uint32), ("device_id", C.c_int32)]


class PfbMfbankPlan(C.Structure):
    _fields_ = [("fft_length", C.c_uint32), ("block_outputs", C.c_uint32), ("num_hypotheses", C.c_uint32),
                ("lds_bytes", C.c_uint32)]


class PfbMfbankCell(C.Structure):
    _fields_ = [("power", C.c_float), ("hypothesis", C.c_int32)]


class PfbCfarConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("element", C.c_uint32), ("method", C.c_uint32), ("block_cells", C.c_uint32),
                ("guard_blocks", C.c_uint32), ("train_blocks", C.c_uint32), ("merge_gap", C.c_uint32),
                ("alpha", C.c_float), ("min_power", C.c_float), ("flags", C.c_uint32), ("device_id", C.c_int32)]


class PfbCfarPlan(C.Structure):
    _fields_ = [("latency_cells", C.c_uint64), ("training_cells", C.c_uint64), ("carry_bytes", C.c_uint64),
                ("sum_kernel", C.c_char * 32)]


class PfbCfarDet(C.Structure):
    _fields_ = [("first_index", C.c_uint64), ("last_index", C.c_uint64), ("peak_index", C.c_uint64),
                ("peak_power", C.c_float), ("noise", C.c_float), ("hypothesis", C.c_int32), ("cells_over", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class PfbCfarStats(C.Structure):
    _fields_ = [("cells_in", C.c_uint64), ("cells_decided", C.c_uint64), ("cells_over", C.c_uint64),
                ("cells_without_noise", C.c_uint64), ("detections", C.c_uint64), ("dropped", C.c_uint64),
                ("open_run", C.c_uint64)]


class PfbPdConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("pri", C.c_uint32), ("origin", C.c_uint64), ("num_gates", C.c_uint32),
                ("num_pulses", C.c_uint32), ("doppler_length", C.c_uint32), ("output", C.c_uint32),
                ("window", C.POINTER(C.c_float)), ("flags", C.c_uint32), ("device_id", C.c_int32)]


class PfbPdPlan(C.Structure):
    _fields_ = [("doppler_length", C.c_uint32), ("tile_gates", C.c_uint32), ("carry_bytes", C.c_uint64),
                ("cpi_samples", C.c_uint64), ("cpi_outputs", C.c_uint64), ("kernel", C.c_char * 32)]


class PfbFoldConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("bin_cells", C.c_uint32), ("num_periods", C.c_uint32),
                ("periods", C.POINTER(C.c_uint32)), ("flags", C.c_uint32), ("device_id", C.c_int32)]


class PfbFoldPlan(C.Structure):
    _fields_ = [("profile_bytes", C.c_uint64), ("total_bins", C.c_uint64), ("max_bins", C.c_uint32),
                ("kernel", C.c_char * 32)]


class PfbFoldScore(C.Structure):
    _fields_ = [("period", C.c_uint32), ("num_bins", C.c_uint32), ("bins_used", C.c_uint32), ("peak_bin", C.c_uint32),
                ("peak_cells", C.c_uint32), ("reserved", C.c_uint32), ("peak_sum", C.c_float), ("peak_mean", C.c_float),
                ("sum_means", C.c_double), ("sum_sq_means", C.c_double), ("cells", C.c_uint64)]


class PfbQfoldConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("bin_cells", C.c_uint32), ("num_periods", C.c_uint32), ("flags", C.c_uint32),
                ("periods_q32", C.POINTER(C.c_uint64)), ("device_id", C.c_int32), ("reserved", C.c_uint32)]


class PfbQfoldPlan(C.Structure):
    _fields_ = [("profile_bytes", C.c_uint64), ("total_bins", C.c_uint64), ("max_bins", C.c_uint32),
                ("kernel", C.c_char * 32)]


class PfbQfoldScore(C.Structure):
    _fields_ = [("period_q32", C.c_uint64), ("num_bins", C.c_uint32), ("bins_used", C.c_uint32), ("peak_bin", C.c_uint32),
                ("reserved", C.c_uint32), ("peak_cells", C.c_uint64), ("peak_sum", C.c_float), ("peak_mean", C.c_float),
                ("sum_means", C.c_double), ("sum_sq_means", C.c_double), ("cells", C.c_uint64)]


class PfbRegridConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("row_samples", C.c_uint32), ("period_q32", C.c_uint64),
                ("origin", C.c_uint64), ("elem_bytes", C.c_uint32), ("flags", C.c_uint32), ("device_id", C.c_int32),
                ("reserved", C.c_uint32)]


class PfbRdcfarConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("rows", C.c_uint32), ("gates", C.c_uint32), ("pitch", C.c_uint32),
                ("doppler_half_width", C.c_uint32), ("guard_gates", C.c_uint32), ("train_gates", C.c_uint32),
                ("peak_half_width", C.c_uint32), ("method", C.c_uint32), ("alpha", C.c_float), ("min_power", C.c_float),
                ("flags", C.c_uint32), ("device_id", C.c_int32)]


class PfbRdcfarPlan(C.Structure):
    _fields_ = [("training_cells", C.c_uint64), ("tile_rows", C.c_uint32), ("tile_gates", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("reserved", C.c_uint32), ("kernel", C.c_char * 32)]


class PfbRdcfarDet(C.Structure):
    _fields_ = [("map", C.c_uint64), ("row", C.c_uint32), ("gate", C.c_uint32), ("power", C.c_float),
                ("noise", C.c_float), ("training_cells", C.c_uint32), ("flags", C.c_uint32)]


class PfbRdcfarStats(C.Structure):
    _fields_ = [("maps_in", C.c_uint64), ("cells_over", C.c_uint64), ("cells_without_noise", C.c_uint64),
                ("detections", C.c_uint64), ("dropped", C.c_uint64)]


class PfbOscfarConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("rows", C.c_uint32), ("gates", C.c_uint32), ("pitch", C.c_uint32),
                ("doppler_half_width", C.c_uint32), ("guard_gates", C.c_uint32), ("train_gates", C.c_uint32),
                ("peak_half_width", C.c_uint32), ("rank", C.c_uint32), ("alpha", C.c_float), ("min_power", C.c_float),
                ("flags", C.c_uint32), ("device_id", C.c_int32)]


class PfbOscfarPlan(C.Structure):
    _fields_ = [("training_cells", C.c_uint64), ("tile_rows", C.c_uint32), ("tile_gates", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("reserved", C.c_uint32), ("kernel", C.c_char * 32)]


class PfbDeintConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_period", C.c_uint32), ("max_period", C.c_uint32),
                ("bin_ticks", C.c_uint32), ("max_level", C.c_uint32), ("detect_percent", C.c_uint32),
                ("min_pulses", C.c_uint32), ("max_missing", C.c_uint32), ("tolerance", C.c_uint32),
                ("fill_percent", C.c_uint32), ("max_emitters", C.c_uint32), ("flags", C.c_uint32),
                ("device_id", C.c_int32)]


class PfbDeintPlan(C.Structure):
    _fields_ = [("scratch_bytes", C.c_uint64), ("num_bins", C.c_uint32), ("lds_bins", C.c_uint32),
                ("tile_pulses", C.c_uint32), ("lds_bytes", C.c_uint32), ("successor_threads", C.c_uint32),
                ("reserved", C.c_uint32), ("histogram_kernel", C.c_char * 32), ("successor_kernel", C.c_char * 32),
                ("marking_kernel", C.c_char * 32)]


class PfbDeintEmitter(C.Structure):
    _fields_ = [("first_tick", C.c_uint64), ("last_tick", C.c_uint64), ("period", C.c_double), ("pulses", C.c_uint32),
                ("periods", C.c_uint32), ("bin", C.c_uint32), ("candidate_period", C.c_uint32),
                ("first_pulse", C.c_uint32), ("hist_count", C.c_uint32)]


class PfbDeintStats(C.Structure):
    _fields_ = [("rounds", C.c_uint64), ("candidates_tried", C.c_uint64), ("candidates_refused", C.c_uint64),
                ("pulses_assigned", C.c_uint64)]


class PfbAssocItem(C.Structure):
    _fields_ = [("start", C.c_uint64), ("length", C.c_uint32), ("cell", C.c_int32), ("weight", C.c_float),
                ("reserved", C.c_uint32)]


class PfbAssocConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("cell_reach", C.c_uint32), ("slack_ticks", C.c_uint32),
                ("window_items", C.c_uint32), ("flags", C.c_uint32), ("device_id", C.c_int32)]


class PfbAssocPlan(C.Structure):
    _fields_ = [("scratch_bytes", C.c_uint64), ("tile_items", C.c_uint32), ("lds_window", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("reserved", C.c_uint32), ("link_kernel", C.c_char * 32),
                ("component_kernel", C.c_char * 32), ("record_kernel", C.c_char * 32)]


class PfbAssocGroup(C.Structure):
    _fields_ = [("first_tick", C.c_uint64), ("end_tick", C.c_uint64), ("length_sum", C.c_uint64),
                ("members", C.c_uint32), ("first_item", C.c_uint32), ("best_item", C.c_uint32), ("best_cell", C.c_int32),
                ("cell_lo", C.c_int32), ("cell_hi", C.c_int32)]


class PfbAssocStats(C.Structure):
    _fields_ = [("groups", C.c_uint64), ("edges", C.c_uint64), ("clipped", C.c_uint64), ("largest_group", C.c_uint64),
                ("linked_items", C.c_uint64), ("rounds", C.c_uint64)]


class PfbClusterItem(C.Structure):
    _fields_ = [("u", C.c_int32), ("v", C.c_int32)]


class PfbClusterConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("cells_u", C.c_uint32), ("cells_v", C.c_uint32), ("reach_u", C.c_uint32),
                ("reach_v", C.c_uint32), ("min_cell_count", C.c_uint32), ("min_pulses", C.c_uint32),
                ("flags", C.c_uint32), ("device_id", C.c_int32)]


class PfbClusterPlan(C.Structure):
    _fields_ = [("scratch_bytes", C.c_uint64), ("cells", C.c_uint32), ("lds_cells", C.c_uint32),
                ("hist_tile", C.c_uint32), ("label_tile", C.c_uint32), ("part_tile", C.c_uint32),
                ("block_u", C.c_uint32), ("block_v", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("max_clusters", C.c_uint32), ("reserved", C.c_uint32), ("histogram_kernel", C.c_char * 32),
                ("component_kernel", C.c_char * 32), ("partition_kernel", C.c_char * 32)]


class PfbClusterGroup(C.Structure):
    _fields_ = [("root_u", C.c_int32), ("root_v", C.c_int32), ("pulses", C.c_uint32), ("cells", C.c_uint32),
                ("u_min", C.c_int32), ("u_max", C.c_int32), ("v_min", C.c_int32), ("v_max", C.c_int32),
                ("sum_u", C.c_int64), ("sum_v", C.c_int64), ("peak_u", C.c_int32), ("peak_v", C.c_int32),
                ("peak_count", C.c_uint32), ("first_item", C.c_uint32)]


class PfbClusterStats(C.Structure):
    _fields_ = [("outside", C.c_uint64), ("unassigned", C.c_uint64), ("dense_cells", C.c_uint64),
                ("border_cells", C.c_uint64), ("components", C.c_uint64), ("hook_rounds", C.c_uint64)]


class PfbMopConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sample_format", C.c_uint32), ("bit_width", C.c_uint32),
                ("trim_samples", C.c_uint32), ("max_negatives", C.c_uint32), ("device_id", C.c_int32)]


class PfbMopPulse(C.Structure):
    _fields_ = [("start", C.c_uint64), ("length", C.c_uint32), ("column", C.c_uint32)]


class PfbMopRecord(C.Structure):
    _fields_ = [("start", C.c_uint64), ("length", C.c_uint32), ("column", C.c_uint32), ("n", C.c_uint32),
                ("flags", C.c_uint32), ("neg_count", C.c_uint32), ("first_neg", C.c_uint32), ("last_neg", C.c_uint32),
                ("peak_index", C.c_uint32), ("negs_listed", C.c_uint32), ("reserved", C.c_uint32),
                ("energy", C.c_double), ("peak_power", C.c_double), ("s1_re", C.c_double), ("s1_im", C.c_double),
                ("s2_re", C.c_double), ("s2_im", C.c_double)]


class PfbMopPlan(C.Structure):
    _fields_ = [("scratch_bytes", C.c_uint64), ("group_min", C.c_uint32), ("split_min", C.c_uint32),
                ("part_samples", C.c_uint32), ("grid_cap", C.c_uint32), ("threads", C.c_uint32),
                ("slice_pulses", C.c_uint32), ("split_slots", C.c_uint32), ("stage_bytes", C.c_uint32),
                ("wave_kernel", C.c_char * 32), ("group_kernel", C.c_char * 32), ("split_kernel", C.c_char * 32),
                ("join_kernel", C.c_char * 32)]


class PfbMopFigure(C.Structure):
    _fields_ = [("freq_hz", C.c_double), ("rate_hz_per_s", C.c_double), ("extent_hz", C.c_double),
                ("mean_power", C.c_double), ("flips", C.c_double), ("kind", C.c_uint32), ("reserved", C.c_uint32)]


class PfbFastPlanDesc(C.Structure):
    _fields_ = [
        ("M", C.c_int), ("P", C.c_int), ("D", C.c_int), ("sample_format", C.c_int), ("variant", C.c_int),
        ("name", C.c_char_p), ("default_schedule", C.c_int), ("magnitude_schedule", C.c_int),
        ("chunk_frames", C.c_int), ("channel_major_ok", C.c_int), ("default_frames_per_block", C.c_int),
        ("threads", C.c_int),
    ]


class PfbLaunchReport(C.Structure):
    _fields_ = [
        ("fused", C.c_int), ("schedule", C.c_int), ("frames_per_block", C.c_int), ("xcd_remap", C.c_int),
        ("by_slabs", C.c_int), ("reserved", C.c_int), ("frames", C.c_uint64), ("runs", C.c_uint64),
        ("slab_frames", C.c_uint64),
    ]


class PfbLaunchRequest(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("schedule", C.c_int), ("frames_per_block", C.c_int), ("xcd_remap", C.c_int),
        ("channel_major", C.c_int), ("magnitude", C.c_int), ("num_cus", C.c_int), ("slab_frames", C.c_int64),
    ]


class PfbKernelEntry(C.Structure):
    _fields_ = [
        ("schedule", C.c_int), ("threads", C.c_int), ("dyn_lds", C.c_uint32), ("reserved", C.c_int),
        ("blocks", C.c_uint64), ("kernel", C.c_uint64), ("_tag", C.c_char_p),
    ]

    @property
    def tag(self) -> str:
        return (self._tag or b"").decode()

    def fields(self) -> tuple:
        """every field, for comparing two entries"""
        return (self.schedule, self.threads, self.dyn_lds, self.blocks, self.kernel, self.tag)


class PfbEntryRequest(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("plan_index", C.c_int), ("launch", PfbLaunchRequest), ("tile_waves", C.c_int),
        ("nontemporal", C.c_int), ("grid", C.c_int), ("experiment", C.c_int), ("out_aligned16", C.c_int),
        ("reserved", C.c_int), ("frames", C.c_uint64),
    ]


PFB_PDW_MATLAB_QUIRKS = 1        # phase(toa:jj) linear-indexes column 1 (create_pdws_channelized.m:114)
PFB_PDW_CHANNEL_MAJOR = 2
PFB_PDW_BINFREQ_UNSHIFTED = 4    # binFreqs(bin) from the FFT-ordered list (:42/:80 if centerFrequencies is unshifted; unpinned)

# int exchange(void* user, const void* d_send, void* d_recv, size_t bytes, int send_to, int recv_from, void* hip_stream)
HALO_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p)


class PfbShardConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("rank", C.c_int32), ("world", C.c_int32), ("ring", C.c_uint32),
                ("exchange", HALO_EXCHANGE_FN), ("user", C.c_void_p)]


class PfbIqInfo(C.Structure):
    _fields_ = [
        ("packet", PfbIqPacket), ("file_format", C.c_int32), ("header_bytes", C.c_uint32),
        ("bytes_per_sample", C.c_uint32), ("sample_format", C.c_uint32), ("rx_gain_as_read", C.c_double),
    ]


# every symbol include/pfb_channelizer.h + include/pfb_iq_packet.h declare: the drop-in boundary
EXPORTS = (
    "pfb_create", "pfb_destroy", "pfb_reset", "pfb_set_stream", "pfb_process", "pfb_process_async", "pfb_sync", "pfb_process_iq_file",
    "pfb_frames_for", "pfb_history_samples", "pfb_prime", "pfb_get_state", "pfb_set_state", "pfb_set_frame_index",
    "pfb_get_frame_index", "pfb_center_frequencies", "pfb_design_prototype", "pfb_strerror",
    "pfb_last_error_detail", "pfb_abi_version", "pfb_device_count", "pfb_set_option", "pfb_last_kernel", "pfb_get_device",
    "pfb_get_kernel_times", "pfb_host_alloc", "pfb_host_free", "pfb_pdw_extract", "pfb_pdw_extract_raw", "pfb_pdw_from_iq_file", "pfb_pdw_raw_from_iq_file", "pfb_pdw_last_error_detail", "pfb_pdw_release_workspace", "pfb_pdw_last_noise_floor_path",
    "pfb_iq_parse_header", "pfb_iq_fill_packet", "pfb_iq_filename",
    "pfb_shard_attach", "pfb_halo_samples", "pfb_shard_head_frames", "pfb_halo_recv_buffer", "pfb_process_shard_async",
    "pfb_center_frequencies_ordered",
    "pfb_stft_create", "pfb_stft_destroy", "pfb_stft_reset", "pfb_stft_set_stream", "pfb_stft_process",
    "pfb_stft_process_async", "pfb_stft_sync", "pfb_stft_frames_for", "pfb_stft_process_iq_file", "pfb_stft_axes",
    "pfb_stft_last_kernel", "pfb_stft_get_device",
    "pfb_dwell_analyze", "pfb_dwell_from_iq_file", "pfb_event_fit", "pfb_event_next",
    "pfb_synth_describe", "pfb_synth_create", "pfb_synth_destroy", "pfb_synth_set_stream", "pfb_synth_generate",
    "pfb_synth_generate_async", "pfb_synth_sync", "pfb_synth_get_device", "pfb_synth_write_iq_file",
    "pfb_iq_serialize_header",
    "pfb_trace_create", "pfb_trace_destroy", "pfb_trace_reset", "pfb_trace_set_stream", "pfb_trace_sync",
    "pfb_trace_get_device", "pfb_trace_bins_for", "pfb_trace_envelope", "pfb_trace_envelope_async", "pfb_trace_flush",
    "pfb_trace_samples", "pfb_trace_choose_bin", "pfb_trace_envelope_from_iq_file",
    "pfb_mf_describe", "pfb_mf_create", "pfb_mf_destroy", "pfb_mf_reset", "pfb_mf_set_stream", "pfb_mf_sync",
    "pfb_mf_get_device", "pfb_mf_outputs_for", "pfb_mf_next_index", "pfb_mf_process", "pfb_mf_process_async",
    "pfb_mf_process_iq_file", "pfb_mf_last_kernel",
    "pfb_wf_create", "pfb_wf_destroy", "pfb_wf_reset", "pfb_wf_set_stream", "pfb_wf_sync", "pfb_wf_get_device",
    "pfb_wf_bins_for", "pfb_wf_process", "pfb_wf_process_async", "pfb_wf_flush", "pfb_wf_choose_bin",
    "pfb_wf_from_channelizer_iq_file", "pfb_wf_from_stft_iq_file",
    "pfb_chsyn_describe", "pfb_chsyn_create", "pfb_chsyn_destroy", "pfb_chsyn_reset", "pfb_chsyn_set_stream",
    "pfb_chsyn_sync", "pfb_chsyn_get_device", "pfb_chsyn_set_frame_index", "pfb_chsyn_get_frame_index",
    "pfb_chsyn_samples_for", "pfb_chsyn_set_weights", "pfb_chsyn_process", "pfb_chsyn_process_async",
    "pfb_chsyn_last_kernel",
    "pfb_mfbank_describe", "pfb_mfbank_frequencies", "pfb_mfbank_create", "pfb_mfbank_destroy", "pfb_mfbank_reset",
    "pfb_mfbank_set_stream", "pfb_mfbank_sync", "pfb_mfbank_get_device", "pfb_mfbank_outputs_for",
    "pfb_mfbank_next_index", "pfb_mfbank_process", "pfb_mfbank_process_async", "pfb_mfbank_process_iq_file",
    "pfb_mfbank_last_kernel",
    "pfb_cfar_describe", "pfb_cfar_alpha", "pfb_cfar_create", "pfb_cfar_destroy", "pfb_cfar_reset", "pfb_cfar_set_stream",
    "pfb_cfar_sync", "pfb_cfar_get_device", "pfb_cfar_next_index", "pfb_cfar_get_stats", "pfb_cfar_process",
    "pfb_cfar_flush", "pfb_cfar_process_async", "pfb_cfar_to_pdw", "pfb_cfar_last_kernel",
    "pfb_pd_describe", "pfb_pd_doppler_frequencies", "pfb_pd_create", "pfb_pd_destroy", "pfb_pd_reset",
    "pfb_pd_set_stream", "pfb_pd_sync", "pfb_pd_get_device", "pfb_pd_cpis_for", "pfb_pd_next_index", "pfb_pd_set_index",
    "pfb_pd_process", "pfb_pd_process_async", "pfb_pd_flush", "pfb_pd_last_kernel",
    "pfb_fold_describe", "pfb_fold_counts", "pfb_fold_create", "pfb_fold_destroy", "pfb_fold_reset",
    "pfb_fold_set_stream", "pfb_fold_sync", "pfb_fold_get_device", "pfb_fold_next_index", "pfb_fold_process",
    "pfb_fold_process_async", "pfb_fold_scores", "pfb_fold_profile", "pfb_fold_last_kernel",
    "pfb_cluster_describe", "pfb_cluster_create", "pfb_cluster_destroy", "pfb_cluster_set_stream", "pfb_cluster_sync",
    "pfb_cluster_get_device", "pfb_cluster_run", "pfb_cluster_histogram", "pfb_cluster_cell_roots", "pfb_cluster_gather",
    "pfb_cluster_last_kernel", "pfb_cluster_get_stats", "pfb_cluster_items_from_pdws",
    "pfb_qfold_describe", "pfb_qfold_counts", "pfb_qfold_create", "pfb_qfold_destroy", "pfb_qfold_reset",
    "pfb_qfold_set_index", "pfb_qfold_set_stream", "pfb_qfold_sync", "pfb_qfold_get_device", "pfb_qfold_next_index",
    "pfb_qfold_process", "pfb_qfold_process_async", "pfb_qfold_scores", "pfb_qfold_profile", "pfb_qfold_last_kernel",
    "pfb_regrid_create", "pfb_regrid_destroy", "pfb_regrid_reset", "pfb_regrid_set_index", "pfb_regrid_set_stream",
    "pfb_regrid_sync", "pfb_regrid_get_device", "pfb_regrid_next_index", "pfb_regrid_outputs_for", "pfb_regrid_process",
    "pfb_regrid_process_async", "pfb_regrid_doppler_frequencies",
    "pfb_assoc_describe", "pfb_assoc_create", "pfb_assoc_destroy", "pfb_assoc_set_stream", "pfb_assoc_sync",
    "pfb_assoc_get_device", "pfb_assoc_run", "pfb_assoc_links", "pfb_assoc_last_kernel", "pfb_assoc_get_stats",
    "pfb_assoc_items_from_pdws",
    "pfb_rdcfar_describe", "pfb_rdcfar_create", "pfb_rdcfar_destroy", "pfb_rdcfar_reset", "pfb_rdcfar_set_stream",
    "pfb_rdcfar_sync", "pfb_rdcfar_get_device", "pfb_rdcfar_next_map", "pfb_rdcfar_get_stats", "pfb_rdcfar_process",
    "pfb_rdcfar_process_async", "pfb_rdcfar_to_pdw", "pfb_rdcfar_last_kernel",
    "pfb_oscfar_describe", "pfb_oscfar_alpha", "pfb_oscfar_create", "pfb_oscfar_destroy", "pfb_oscfar_reset",
    "pfb_oscfar_set_stream", "pfb_oscfar_sync", "pfb_oscfar_get_device", "pfb_oscfar_next_map", "pfb_oscfar_get_stats",
    "pfb_oscfar_process", "pfb_oscfar_process_async", "pfb_oscfar_last_kernel",
    "pfb_deint_describe", "pfb_deint_create", "pfb_deint_destroy", "pfb_deint_set_stream", "pfb_deint_sync",
    "pfb_deint_get_device", "pfb_deint_run", "pfb_deint_histogram", "pfb_deint_successors", "pfb_deint_last_kernel",
    "pfb_deint_get_stats", "pfb_deint_ticks_from_toa",
    "pfb_mop_describe", "pfb_mop_create", "pfb_mop_destroy", "pfb_mop_set_stream", "pfb_mop_sync", "pfb_mop_get_device",
    "pfb_mop_measure", "pfb_mop_measure_async", "pfb_mop_last_kernel", "pfb_mop_figures", "pfb_mop_pulses_from_pdw",
)
# include/pfb_channelizer_dev.h: measurement yardsticks and the ABI self test (bench.py, tools/, tests/)
DEV_EXPORTS = ("pfb_measure_stream_copy", "pfb_measure_mix_copy", "pfb_selftest_exception_guard", "pfb_stft_set_experiment",
               "pfb_fold_set_tier", "pfb_deint_set_tier", "pfb_mop_set_tier", "pfb_qfold_set_tier",
               "pfb_assoc_set_tier", "pfb_cluster_set_tier",
               "pfb_fast_plan_count", "pfb_fast_plan_info", "pfb_last_launch", "pfb_plan_launch", "pfb_last_entry", "pfb_plan_entry")

_lib = None


class PfbError(RuntimeError):
    def __init__(self, status: int, where: str):
        lib = load()
        msg = lib.pfb_strerror(status).decode()
        detail = lib.pfb_last_error_detail().decode()
        super().__init__(f"{where}: {msg} ({status})" + (f" [{detail}]" if detail else ""))
        self.status = status


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own libamdhip64; two HIP runtimes in one process cannot both own the
    # GPU ("No HIP GPUs are available" for whichever comes second).  If PyTorch is installed, let it
    # load its runtime first: our library's libamdhip64.so.7 dependency then binds to that same copy,
    # and torch tensors / streams can be handed straight to the C ABI.
    if "torch" not in sys.modules and os.environ.get("PFB_NO_TORCH_PRELOAD") is None:
        import importlib.util
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m sdr_channelizer_amd.build` "
            "(hipcc, gfx950). The channelizer has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, u64, u32, i32, i64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64
    lib.pfb_create.argtypes = [C.POINTER(PfbConfig), C.POINTER(vp)]
    lib.pfb_destroy.argtypes = [vp]
    lib.pfb_reset.argtypes = [vp]
    lib.pfb_set_stream.argtypes = [vp, vp]
    lib.pfb_process.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32]
    lib.pfb_process_async.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    lib.pfb_sync.argtypes = [vp]
    lib.pfb_process_iq_file.argtypes = [vp, C.c_char_p, vp, u64, C.POINTER(u64), C.POINTER(PfbIqInfo)]
    lib.pfb_frames_for.argtypes = [vp, u64, C.POINTER(u64)]
    lib.pfb_history_samples.argtypes = [vp]
    lib.pfb_history_samples.restype = u64
    lib.pfb_prime.argtypes = [vp, vp, u64, u32]
    lib.pfb_get_state.argtypes = [vp, vp, C.POINTER(C.c_size_t)]
    lib.pfb_set_state.argtypes = [vp, vp, C.c_size_t]
    lib.pfb_set_frame_index.argtypes = [vp, u64]
    lib.pfb_get_frame_index.argtypes = [vp, C.POINTER(u64)]
    lib.pfb_center_frequencies.argtypes = [u32, C.c_double, C.POINTER(C.c_double)]
    lib.pfb_center_frequencies_ordered.argtypes = [u32, C.c_double, u32, C.POINTER(C.c_double)]
    lib.pfb_selftest_exception_guard.argtypes = [C.c_int]
    lib.pfb_shard_attach.argtypes = [vp, C.POINTER(PfbShardConfig)]
    lib.pfb_halo_samples.argtypes = [vp]
    lib.pfb_halo_samples.restype = u64
    lib.pfb_shard_head_frames.argtypes = [vp]
    lib.pfb_shard_head_frames.restype = u64
    lib.pfb_halo_recv_buffer.argtypes = [vp]
    lib.pfb_halo_recv_buffer.restype = C.c_void_p
    lib.pfb_process_shard_async.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    lib.pfb_design_prototype.argtypes = [u32, u32, C.c_double, C.POINTER(C.c_float)]
    lib.pfb_strerror.argtypes = [C.c_int]
    lib.pfb_strerror.restype = C.c_char_p
    lib.pfb_last_error_detail.restype = C.c_char_p
    lib.pfb_set_option.argtypes = [vp, C.c_int, i64]
    lib.pfb_last_kernel.argtypes = [vp]
    lib.pfb_last_kernel.restype = C.c_char_p
    lib.pfb_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_get_kernel_times.argtypes = [vp, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
    lib.pfb_host_alloc.argtypes = [C.c_size_t]
    lib.pfb_host_alloc.restype = C.c_void_p
    lib.pfb_host_free.argtypes = [vp]
    lib.pfb_host_free.restype = None
    lib.pfb_pdw_extract.argtypes = [vp, u64, u32, u32, C.c_double, C.c_double, C.c_double, C.c_double, u32,
                                    C.POINTER(PfbPdw), u64, C.POINTER(u64), C.POINTER(C.c_double), u32, i32, vp]
    lib.pfb_pdw_from_iq_file.argtypes = [vp, C.c_char_p, C.c_double, u32, C.POINTER(PfbPdw), u64, C.POINTER(u64),
                                         C.POINTER(C.c_double), C.POINTER(PfbIqInfo)]
    lib.pfb_pdw_from_iq_file.restype = C.c_int
    lib.pfb_pdw_raw_from_iq_file.argtypes = [C.c_char_p, C.c_double, C.c_double, C.POINTER(PfbPdw), u64, C.POINTER(u64),
                                             C.POINTER(C.c_double), C.POINTER(PfbIqInfo), C.c_int32]
    lib.pfb_pdw_raw_from_iq_file.restype = C.c_int
    lib.pfb_pdw_extract_raw.argtypes = [vp, u64, u32, u32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                        C.POINTER(PfbPdw), u64, C.POINTER(u64), C.POINTER(C.c_double), u32, i32, vp]
    lib.pfb_pdw_last_error_detail.restype = C.c_char_p
    lib.pfb_pdw_release_workspace.argtypes = [C.c_int32]
    lib.pfb_pdw_release_workspace.restype = C.c_int
    lib.pfb_pdw_last_noise_floor_path.restype = C.c_int
    lib.pfb_measure_stream_copy.argtypes = [C.c_int, u64, C.c_int, C.POINTER(C.c_double)]
    lib.pfb_measure_mix_copy.argtypes = [C.c_int, u64, u32, u32, C.c_int, C.POINTER(C.c_double)]
    lib.pfb_iq_parse_header.argtypes = [vp, C.c_size_t, C.POINTER(PfbIqInfo)]
    lib.pfb_iq_fill_packet.argtypes = [C.POINTER(PfbIqPacket), u32, u64, u32, u32, C.c_float, u32, u32,
                                       C.c_char_p, C.c_char_p, C.c_double]
    lib.pfb_iq_fill_packet.restype = None
    lib.pfb_iq_filename.argtypes = [i64, C.c_char_p, C.c_int]
    lib.pfb_stft_create.argtypes = [C.POINTER(PfbStftConfig), C.POINTER(vp)]
    lib.pfb_stft_destroy.argtypes = [vp]
    lib.pfb_stft_reset.argtypes = [vp]
    lib.pfb_stft_set_stream.argtypes = [vp, vp]
    lib.pfb_stft_process.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32]
    lib.pfb_stft_process_async.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    lib.pfb_stft_sync.argtypes = [vp]
    lib.pfb_stft_frames_for.argtypes = [vp, u64, C.POINTER(u64)]
    lib.pfb_stft_process_iq_file.argtypes = [vp, C.c_char_p, vp, u64, C.POINTER(u64), C.POINTER(PfbIqInfo)]
    lib.pfb_stft_axes.argtypes = [u32, u32, u32, C.c_double, u32, u64, u64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.pfb_stft_last_kernel.argtypes = [vp]
    lib.pfb_stft_last_kernel.restype = C.c_char_p
    lib.pfb_stft_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_dwell_analyze.argtypes = [C.POINTER(PfbDwellConfig), vp, u64, C.POINTER(PfbPdw), u64, C.POINTER(u64),
                                      C.POINTER(PfbDwellStats), vp]
    lib.pfb_dwell_from_iq_file.argtypes = [C.c_char_p, C.POINTER(PfbDwellConfig), C.POINTER(PfbPdw), u64, C.POINTER(u64),
                                           C.POINTER(PfbDwellStats), C.POINTER(PfbIqInfo)]
    lib.pfb_event_fit.argtypes = [C.POINTER(PfbPdw), u64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_double)]
    lib.pfb_event_next.argtypes = [C.POINTER(C.c_double), u64, u32, C.POINTER(C.c_double), C.POINTER(i32)]
    lib.pfb_synth_describe.argtypes = [C.POINTER(PfbSynthConfig), C.POINTER(PfbSynthParams), C.POINTER(i64)]
    lib.pfb_synth_create.argtypes = [C.POINTER(PfbSynthConfig), C.POINTER(vp)]
    lib.pfb_synth_destroy.argtypes = [vp]
    lib.pfb_synth_set_stream.argtypes = [vp, vp]
    lib.pfb_synth_generate.argtypes = [vp, u64, u64, vp, u32]
    lib.pfb_synth_generate_async.argtypes = [vp, u64, u64, vp]
    lib.pfb_synth_sync.argtypes = [vp]
    lib.pfb_synth_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_synth_write_iq_file.argtypes = [vp, C.c_char_p, C.c_int, u64, u32, C.POINTER(PfbIqPacket)]
    lib.pfb_iq_serialize_header.argtypes = [C.POINTER(PfbIqPacket), C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.pfb_trace_create.argtypes = [C.POINTER(PfbTraceConfig), C.POINTER(vp)]
    lib.pfb_trace_destroy.argtypes = [vp]
    lib.pfb_trace_reset.argtypes = [vp]
    lib.pfb_trace_set_stream.argtypes = [vp, vp]
    lib.pfb_trace_sync.argtypes = [vp]
    lib.pfb_trace_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_trace_bins_for.argtypes = [vp, u64, C.POINTER(u64)]
    lib.pfb_trace_envelope.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32]
    lib.pfb_trace_envelope_async.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    lib.pfb_trace_flush.argtypes = [vp, C.POINTER(PfbTraceBin), C.POINTER(i32)]
    lib.pfb_trace_samples.argtypes = [vp, vp, u64, vp, vp, u32]
    lib.pfb_trace_choose_bin.argtypes = [u64, u32, C.POINTER(u32)]
    lib.pfb_trace_envelope_from_iq_file.argtypes = [C.c_char_p, u32, vp, u64, C.POINTER(u64), C.POINTER(u32),
                                                    C.POINTER(PfbIqInfo), i32]
    lib.pfb_mf_describe.argtypes = [C.POINTER(PfbMfConfig), C.POINTER(PfbMfPlan)]
    lib.pfb_mf_create.argtypes = [C.POINTER(PfbMfConfig), C.POINTER(vp)]
    lib.pfb_mf_destroy.argtypes = [vp]
    lib.pfb_mf_reset.argtypes = [vp]
    lib.pfb_mf_set_stream.argtypes = [vp, vp]
    lib.pfb_mf_sync.argtypes = [vp]
    lib.pfb_mf_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_mf_outputs_for.argtypes = [vp, u64, C.POINTER(u64)]
    lib.pfb_mf_next_index.argtypes = [vp, C.POINTER(u64)]
    lib.pfb_mf_process.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32]
    lib.pfb_mf_process_async.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    lib.pfb_mf_process_iq_file.argtypes = [vp, C.c_char_p, vp, u64, C.POINTER(u64), C.POINTER(PfbIqInfo)]
    lib.pfb_mf_last_kernel.argtypes = [vp]
    lib.pfb_mf_last_kernel.restype = C.c_char_p
    lib.pfb_wf_create.argtypes = [C.POINTER(PfbWfConfig), C.POINTER(vp)]
    lib.pfb_wf_destroy.argtypes = [vp]
    lib.pfb_wf_reset.argtypes = [vp]
    lib.pfb_wf_set_stream.argtypes = [vp, vp]
    lib.pfb_wf_sync.argtypes = [vp]
    lib.pfb_wf_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_wf_bins_for.argtypes = [vp, u64, C.POINTER(u64)]
    lib.pfb_wf_process.argtypes = [vp, vp, u64, u64, vp, u64, C.POINTER(u64), u32]
    lib.pfb_wf_process_async.argtypes = [vp, vp, u64, u64, vp, u64, C.POINTER(u64)]
    lib.pfb_wf_flush.argtypes = [vp, vp, C.POINTER(u32)]
    lib.pfb_wf_choose_bin.argtypes = [u64, u32, C.POINTER(u32)]
    lib.pfb_wf_from_channelizer_iq_file.argtypes = [vp, C.c_char_p, u32, u64, vp, u64, C.POINTER(u64), C.POINTER(u32),
                                                    C.POINTER(PfbIqInfo)]
    lib.pfb_wf_from_stft_iq_file.argtypes = [vp, C.c_char_p, u32, u64, vp, u64, C.POINTER(u64), C.POINTER(u32),
                                             C.POINTER(PfbIqInfo)]
    lib.pfb_chsyn_describe.argtypes = [C.POINTER(PfbChsynConfig), C.POINTER(PfbChsynPlan)]
    lib.pfb_chsyn_create.argtypes = [C.POINTER(PfbChsynConfig), C.POINTER(vp)]
    lib.pfb_chsyn_destroy.argtypes = [vp]
    lib.pfb_chsyn_reset.argtypes = [vp]
    lib.pfb_chsyn_set_stream.argtypes = [vp, vp]
    lib.pfb_chsyn_sync.argtypes = [vp]
    lib.pfb_chsyn_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_chsyn_set_frame_index.argtypes = [vp, u64]
    lib.pfb_chsyn_get_frame_index.argtypes = [vp, C.POINTER(u64)]
    lib.pfb_chsyn_samples_for.argtypes = [vp, u64, C.POINTER(u64)]
    lib.pfb_chsyn_set_weights.argtypes = [vp, vp]
    lib.pfb_chsyn_process.argtypes = [vp, vp, u64, u64, vp, u64, C.POINTER(u64), u32]
    lib.pfb_chsyn_process_async.argtypes = [vp, vp, u64, u64, vp, u64, C.POINTER(u64)]
    lib.pfb_chsyn_last_kernel.argtypes = [vp]
    lib.pfb_chsyn_last_kernel.restype = C.c_char_p
    lib.pfb_mfbank_describe.argtypes = [C.POINTER(PfbMfbankConfig), C.POINTER(PfbMfbankPlan)]
    lib.pfb_mfbank_frequencies.argtypes = [C.POINTER(PfbMfbankConfig), C.c_double, C.POINTER(C.c_double)]
    lib.pfb_mfbank_create.argtypes = [C.POINTER(PfbMfbankConfig), C.POINTER(vp)]
    lib.pfb_mfbank_destroy.argtypes = [vp]
    lib.pfb_mfbank_reset.argtypes = [vp]
    lib.pfb_mfbank_set_stream.argtypes = [vp, vp]
    lib.pfb_mfbank_sync.argtypes = [vp]
    lib.pfb_mfbank_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_mfbank_outputs_for.argtypes = [vp, u64, C.POINTER(u64)]
    lib.pfb_mfbank_next_index.argtypes = [vp, C.POINTER(u64)]
    lib.pfb_mfbank_process.argtypes = [vp, vp, u64, vp, u64, u64, C.POINTER(u64), u32]
    lib.pfb_mfbank_process_async.argtypes = [vp, vp, u64, vp, u64, u64, C.POINTER(u64)]
    lib.pfb_mfbank_process_iq_file.argtypes = [vp, C.c_char_p, vp, u64, u64, C.POINTER(u64), C.POINTER(PfbIqInfo)]
    lib.pfb_mfbank_last_kernel.argtypes = [vp]
    lib.pfb_mfbank_last_kernel.restype = C.c_char_p
    lib.pfb_cfar_describe.argtypes = [C.POINTER(PfbCfarConfig), C.POINTER(PfbCfarPlan)]
    lib.pfb_cfar_alpha.argtypes = [C.c_double, u64, C.POINTER(C.c_double)]
    lib.pfb_cfar_create.argtypes = [C.POINTER(PfbCfarConfig), C.POINTER(vp)]
    lib.pfb_cfar_destroy.argtypes = [vp]
    lib.pfb_cfar_reset.argtypes = [vp]
    lib.pfb_cfar_set_stream.argtypes = [vp, vp]
    lib.pfb_cfar_sync.argtypes = [vp]
    lib.pfb_cfar_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_cfar_next_index.argtypes = [vp, C.POINTER(u64)]
    lib.pfb_cfar_get_stats.argtypes = [vp, C.POINTER(PfbCfarStats)]
    lib.pfb_cfar_process.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32]
    lib.pfb_cfar_flush.argtypes = [vp, vp, u64, C.POINTER(u64), u32]
    lib.pfb_cfar_process_async.argtypes = [vp, vp, u64, vp, u64, vp]
    lib.pfb_cfar_to_pdw.argtypes = [vp, u64, C.c_double, C.c_double, C.c_double, C.c_double, i32, u32, C.POINTER(PfbPdw)]
    lib.pfb_cfar_last_kernel.argtypes = [vp]
    lib.pfb_cfar_last_kernel.restype = C.c_char_p
    lib.pfb_pd_describe.argtypes = [C.POINTER(PfbPdConfig), C.POINTER(PfbPdPlan)]
    lib.pfb_pd_doppler_frequencies.argtypes = [C.POINTER(PfbPdConfig), C.c_double, C.POINTER(C.c_double)]
    lib.pfb_pd_create.argtypes = [C.POINTER(PfbPdConfig), C.POINTER(vp)]
    lib.pfb_pd_destroy.argtypes = [vp]
    lib.pfb_pd_reset.argtypes = [vp]
    lib.pfb_pd_set_stream.argtypes = [vp, vp]
    lib.pfb_pd_sync.argtypes = [vp]
    lib.pfb_pd_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_pd_cpis_for.argtypes = [vp, u64, C.POINTER(u64)]
    lib.pfb_pd_next_index.argtypes = [vp, C.POINTER(u64)]
    lib.pfb_pd_set_index.argtypes = [vp, u64]
    lib.pfb_pd_process.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32]
    lib.pfb_pd_process_async.argtypes = [vp, vp, u64, vp, u64, vp]
    lib.pfb_pd_flush.argtypes = [vp, vp, u64, C.POINTER(u64), u32]
    lib.pfb_pd_last_kernel.argtypes = [vp]
    lib.pfb_pd_last_kernel.restype = C.c_char_p
    lib.pfb_fold_describe.argtypes = [C.POINTER(PfbFoldConfig), C.POINTER(PfbFoldPlan)]
    lib.pfb_fold_counts.argtypes = [C.POINTER(PfbFoldConfig), u32, u64, C.POINTER(u64)]
    lib.pfb_fold_create.argtypes = [C.POINTER(PfbFoldConfig), C.POINTER(vp)]
    lib.pfb_fold_destroy.argtypes = [vp]
    lib.pfb_fold_reset.argtypes = [vp]
    lib.pfb_fold_set_stream.argtypes = [vp, vp]
    lib.pfb_fold_sync.argtypes = [vp]
    lib.pfb_fold_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_fold_next_index.argtypes = [vp, C.POINTER(u64)]
    lib.pfb_fold_process.argtypes = [vp, vp, u64, u32]
    lib.pfb_fold_process_async.argtypes = [vp, vp, u64]
    lib.pfb_fold_scores.argtypes = [vp, vp, u64, u32]
    lib.pfb_fold_profile.argtypes = [vp, u32, vp, u64, u32]
    lib.pfb_fold_last_kernel.argtypes = [vp]
    lib.pfb_fold_last_kernel.restype = C.c_char_p
    lib.pfb_rdcfar_describe.argtypes = [C.POINTER(PfbRdcfarConfig), C.POINTER(PfbRdcfarPlan)]
    lib.pfb_rdcfar_create.argtypes = [C.POINTER(PfbRdcfarConfig), C.POINTER(vp)]
    lib.pfb_rdcfar_destroy.argtypes = [vp]
    lib.pfb_rdcfar_reset.argtypes = [vp]
    lib.pfb_rdcfar_set_stream.argtypes = [vp, vp]
    lib.pfb_rdcfar_sync.argtypes = [vp]
    lib.pfb_rdcfar_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_rdcfar_next_map.argtypes = [vp, C.POINTER(u64)]
    lib.pfb_rdcfar_get_stats.argtypes = [vp, C.POINTER(PfbRdcfarStats)]
    lib.pfb_rdcfar_process.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32]
    lib.pfb_rdcfar_process_async.argtypes = [vp, vp, u64, vp, u64, vp]
    lib.pfb_rdcfar_to_pdw.argtypes = [vp, u64, C.c_double, C.c_double, C.c_double, u32, u32, u64, u32, u32,
                                      C.POINTER(PfbPdw)]
    lib.pfb_rdcfar_last_kernel.argtypes = [vp]
    lib.pfb_rdcfar_last_kernel.restype = C.c_char_p
    lib.pfb_oscfar_describe.argtypes = [C.POINTER(PfbOscfarConfig), C.POINTER(PfbOscfarPlan)]
    lib.pfb_oscfar_alpha.argtypes = [C.c_double, u64, u64, C.POINTER(C.c_double)]
    lib.pfb_oscfar_create.argtypes = [C.POINTER(PfbOscfarConfig), C.POINTER(vp)]
    lib.pfb_oscfar_destroy.argtypes = [vp]
    lib.pfb_oscfar_reset.argtypes = [vp]
    lib.pfb_oscfar_set_stream.argtypes = [vp, vp]
    lib.pfb_oscfar_sync.argtypes = [vp]
    lib.pfb_oscfar_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_oscfar_next_map.argtypes = [vp, C.POINTER(u64)]
    lib.pfb_oscfar_get_stats.argtypes = [vp, C.POINTER(PfbRdcfarStats)]
    lib.pfb_oscfar_process.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32]
    lib.pfb_oscfar_process_async.argtypes = [vp, vp, u64, vp, u64, vp]
    lib.pfb_oscfar_last_kernel.argtypes = [vp]
    lib.pfb_oscfar_last_kernel.restype = C.c_char_p
    lib.pfb_deint_describe.argtypes = [C.POINTER(PfbDeintConfig), u64, C.POINTER(PfbDeintPlan)]
    lib.pfb_deint_create.argtypes = [C.POINTER(PfbDeintConfig), C.POINTER(vp)]
    lib.pfb_deint_destroy.argtypes = [vp]
    lib.pfb_deint_set_stream.argtypes = [vp, vp]
    lib.pfb_deint_sync.argtypes = [vp]
    lib.pfb_deint_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_deint_run.argtypes = [vp, vp, u64, u32, vp, u64, C.POINTER(u64), vp]
    lib.pfb_deint_histogram.argtypes = [vp, vp, u64, u32, vp, u64]
    lib.pfb_deint_successors.argtypes = [vp, vp, u64, u32, u64, vp, vp, vp]
    lib.pfb_deint_last_kernel.argtypes = [vp]
    lib.pfb_deint_last_kernel.restype = C.c_char_p
    lib.pfb_deint_get_stats.argtypes = [vp, C.POINTER(PfbDeintStats)]
    lib.pfb_deint_ticks_from_toa.argtypes = [vp, u64, u64, C.c_double, C.c_double, vp, vp]
    lib.pfb_mop_describe.argtypes = [C.POINTER(PfbMopConfig), C.POINTER(PfbMopPlan)]
    lib.pfb_mop_create.argtypes = [C.POINTER(PfbMopConfig), C.POINTER(vp)]
    lib.pfb_mop_destroy.argtypes = [vp]
    lib.pfb_mop_set_stream.argtypes = [vp, vp]
    lib.pfb_mop_sync.argtypes = [vp]
    lib.pfb_mop_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_mop_measure.argtypes = [vp, vp, u64, u64, u64, u32, vp, u64, u32, vp, vp]
    lib.pfb_mop_measure_async.argtypes = [vp, vp, u64, u64, u64, vp, u64, vp, vp]
    lib.pfb_mop_last_kernel.argtypes = [vp]
    lib.pfb_mop_last_kernel.restype = C.c_char_p
    lib.pfb_mop_figures.argtypes = [vp, u64, C.c_double, vp]
    lib.pfb_mop_pulses_from_pdw.argtypes = [vp, u64, C.c_double, C.c_double, vp]
    lib.pfb_qfold_describe.argtypes = [C.POINTER(PfbQfoldConfig), C.POINTER(PfbQfoldPlan)]
    lib.pfb_qfold_counts.argtypes = [C.POINTER(PfbQfoldConfig), u32, u64, u64, C.POINTER(u64)]
    lib.pfb_qfold_create.argtypes = [C.POINTER(PfbQfoldConfig), C.POINTER(vp)]
    lib.pfb_qfold_destroy.argtypes = [vp]
    lib.pfb_qfold_reset.argtypes = [vp]
    lib.pfb_qfold_set_index.argtypes = [vp, u64]
    lib.pfb_qfold_set_stream.argtypes = [vp, vp]
    lib.pfb_qfold_sync.argtypes = [vp]
    lib.pfb_qfold_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_qfold_next_index.argtypes = [vp, C.POINTER(u64)]
    lib.pfb_qfold_process.argtypes = [vp, vp, u64, u32]
    lib.pfb_qfold_process_async.argtypes = [vp, vp, u64]
    lib.pfb_qfold_scores.argtypes = [vp, vp, u64, u32]
    lib.pfb_qfold_profile.argtypes = [vp, u32, vp, u64, u32]
    lib.pfb_qfold_last_kernel.argtypes = [vp]
    lib.pfb_qfold_last_kernel.restype = C.c_char_p
    lib.pfb_regrid_create.argtypes = [C.POINTER(PfbRegridConfig), C.POINTER(vp)]
    lib.pfb_regrid_destroy.argtypes = [vp]
    lib.pfb_regrid_reset.argtypes = [vp]
    lib.pfb_regrid_set_index.argtypes = [vp, u64]
    lib.pfb_regrid_set_stream.argtypes = [vp, vp]
    lib.pfb_regrid_sync.argtypes = [vp]
    lib.pfb_regrid_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_regrid_next_index.argtypes = [vp, C.POINTER(u64)]
    lib.pfb_regrid_outputs_for.argtypes = [vp, u64, C.POINTER(u64)]
    lib.pfb_regrid_process.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), u32]
    lib.pfb_regrid_process_async.argtypes = [vp, vp, u64, vp, u64, vp]
    lib.pfb_regrid_doppler_frequencies.argtypes = [u64, u32, C.c_int, C.c_double, C.POINTER(C.c_double)]
    lib.pfb_assoc_describe.argtypes = [C.POINTER(PfbAssocConfig), u64, C.POINTER(PfbAssocPlan)]
    lib.pfb_assoc_create.argtypes = [C.POINTER(PfbAssocConfig), C.POINTER(vp)]
    lib.pfb_assoc_destroy.argtypes = [vp]
    lib.pfb_assoc_set_stream.argtypes = [vp, vp]
    lib.pfb_assoc_sync.argtypes = [vp]
    lib.pfb_assoc_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_assoc_run.argtypes = [vp, vp, u64, u32, vp, u64, C.POINTER(u64), vp]
    lib.pfb_assoc_links.argtypes = [vp, vp, u64, u32, vp, vp]
    lib.pfb_assoc_last_kernel.argtypes = [vp]
    lib.pfb_assoc_last_kernel.restype = C.c_char_p
    lib.pfb_assoc_get_stats.argtypes = [vp, C.POINTER(PfbAssocStats)]
    lib.pfb_assoc_items_from_pdws.argtypes = [vp, u64, C.c_double, C.c_double, vp, vp]
    lib.pfb_assoc_set_tier.argtypes = [vp, C.c_int]
    lib.pfb_cluster_describe.argtypes = [C.POINTER(PfbClusterConfig), u64, C.POINTER(PfbClusterPlan)]
    lib.pfb_cluster_create.argtypes = [C.POINTER(PfbClusterConfig), C.POINTER(vp)]
    lib.pfb_cluster_destroy.argtypes = [vp]
    lib.pfb_cluster_set_stream.argtypes = [vp, vp]
    lib.pfb_cluster_sync.argtypes = [vp]
    lib.pfb_cluster_get_device.argtypes = [vp, C.POINTER(C.c_int)]
    lib.pfb_cluster_run.argtypes = [vp, vp, u64, u32, vp, u64, C.POINTER(u64), vp, vp, vp]
    lib.pfb_cluster_histogram.argtypes = [vp, vp, u64, u32, vp, u64]
    lib.pfb_cluster_cell_roots.argtypes = [vp, vp, u64, u32, vp, u64]
    lib.pfb_cluster_gather.argtypes = [vp, vp, u32, vp, u64, vp]
    lib.pfb_cluster_last_kernel.argtypes = [vp]
    lib.pfb_cluster_last_kernel.restype = C.c_char_p
    lib.pfb_cluster_get_stats.argtypes = [vp, C.POINTER(PfbClusterStats)]
    lib.pfb_cluster_items_from_pdws.argtypes = [vp, u64, u64, C.c_double, C.c_double, C.c_double, vp]
    lib.pfb_cluster_set_tier.argtypes = [vp, C.c_int]
    lib.pfb_fold_set_tier.argtypes = [vp, C.c_int]
    lib.pfb_qfold_set_tier.argtypes = [vp, C.c_int, u64]
    lib.pfb_mop_set_tier.argtypes = [vp, C.c_int, u32, u64]
    lib.pfb_deint_set_tier.argtypes = [vp, C.c_int, C.c_int]
    lib.pfb_stft_set_experiment.argtypes = [vp, C.c_int]
    lib.pfb_fast_plan_count.argtypes = []
    lib.pfb_fast_plan_info.argtypes = [C.c_int, C.POINTER(PfbFastPlanDesc)]
    lib.pfb_last_launch.argtypes = [vp, C.POINTER(PfbLaunchReport)]
    lib.pfb_plan_launch.argtypes = [C.c_int, C.POINTER(PfbLaunchRequest), u64, C.POINTER(PfbLaunchReport)]
    lib.pfb_last_entry.argtypes = [vp, C.POINTER(PfbKernelEntry)]
    lib.pfb_plan_entry.argtypes = [C.POINTER(PfbEntryRequest), C.POINTER(PfbKernelEntry)]
    for name in EXPORTS + DEV_EXPORTS:
        getattr(lib, name)  # AttributeError here = header/library mismatch
    _lib = lib
    return lib


def check(status: int, where: str) -> None:
    if status != PFB_OK:
        raise PfbError(status, where)


def fast_plans() -> list[PfbFastPlanDesc]:
    """Every row of the fused-kernel table, in lookup order (pfb_fast_plan_info; host only)."""
    lib = load()
    rows = []
    for i in range(lib.pfb_fast_plan_count()):
        d = PfbFastPlanDesc()
        check(lib.pfb_fast_plan_info(i, C.byref(d)), "pfb_fast_plan_info")
        rows.append(d)
    return rows


def plan_launch(row: int, frames: int, num_cus: int, schedule: int = -1, frames_per_block: int = 0, xcd_remap: int = -1,
                slab_frames: int = 0, channel_major: bool = False, magnitude: bool = False) -> PfbLaunchReport:
    """What the launch policy decides for row ``row`` of the table, these options and ``frames`` frames
    (pfb_plan_launch; host only): the report a handle stores for that launch."""
    rq = PfbLaunchRequest(C.sizeof(PfbLaunchRequest), schedule, frames_per_block, xcd_remap, int(channel_major),
                          int(magnitude), num_cus, slab_frames)
    rep = PfbLaunchReport()
    check(load().pfb_plan_launch(row, C.byref(rq), frames, C.byref(rep)), "pfb_plan_launch")
    return rep


def plan_entry(row: int, frames: int, num_cus: int, schedule: int = -1, frames_per_block: int = 0, xcd_remap: int = -1,
               slab_frames: int = 0, channel_major: bool = False, magnitude: bool = False, tile_waves: int = 8,
               nontemporal: bool = False, grid: int = 0, experiment: int = 0, out_aligned16: bool = True) -> PfbKernelEntry:
    """The kernel entry row ``row`` of the table resolves these options and ``frames`` frames to (pfb_plan_entry; host
    only): the policy of plan_launch, then the row's select -- what a handle's last_entry holds after that launch."""
    launch = PfbLaunchRequest(C.sizeof(PfbLaunchRequest), schedule, frames_per_block, xcd_remap, int(channel_major),
                              int(magnitude), num_cus, slab_frames)
    rq = PfbEntryRequest(C.sizeof(PfbEntryRequest), row, launch, tile_waves, int(nontemporal), grid, experiment,
                         int(out_aligned16), 0, frames)
    e = PfbKernelEntry()
    check(load().pfb_plan_entry(C.byref(rq), C.byref(e)), "pfb_plan_entry")
    return e
