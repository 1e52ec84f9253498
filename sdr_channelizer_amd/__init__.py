"""MI355X-native polyphase-filterbank channelizer: a drop-in for the channelizer
path of cwozny/sdr_channelizer (see DESIGN.md / INTEGRATION.md).

The arithmetic lives in libpfb_channelizer.so (HIP, gfx950) behind the C ABI of
include/pfb_channelizer.h; this package is the thin host side.
"""
from ._lib import LIB_PATH, PfbError  # noqa: F401
from .associate import (ASSOC_ITEM_DTYPE, GROUP_DTYPE, PulseAssociator, associate, associate_pdws,  # noqa: F401
                        describe_associator, fuse_pdws)
from .cfar import (Cfar, cfar_alpha, detect, detect_pulses, detections_to_pdws,  # noqa: F401
                   pulse_detections_from_iq_file)
from .channelizer import Channelizer, center_frequencies, design_prototype, pinned_empty  # noqa: F401
from .cluster import (CLUSTER_GROUP_DTYPE, CLUSTER_ITEM_DTYPE, PulseClusterer, cluster_pdws, cluster_pulses,  # noqa: F401
                      deinterleave_clustered, deinterleave_clustered_figures, describe_clusterer)
from .cluster import items_from_pdws as cluster_items_from_pdws  # noqa: F401
from .deinterleave import (EMITTER_DTYPE, Deinterleaver, deinterleave, deinterleave_detections,  # noqa: F401
                           deinterleave_pdws, describe_deinterleaver, merge_emitters, ticks_from_toa)
from .event import DwellStats, EventPredictor, analyze_dwell, dwell_from_iq_file, fit_event, next_event  # noqa: F401
from .matched_filter import (MatchedFilter, compress, compress_iq_file, pulse_delay_from_iq_files,  # noqa: F401
                             replica_from_pulse_train)
from .mf_bank import (MatchedFilterBank, bank_frequencies, compress_bank,  # noqa: F401
                      pulse_delay_and_offset_from_iq_files)
from .os_cfar import OsCfar, detect_maps_os, os_cfar_alpha  # noqa: F401
from .pri_fine import (QSCORE_DTYPE, FinePriFold, Regrid, describe_fine_fold, detect_pulse_train_fine,  # noqa: F401
                       find_pri_fine, period_q32, period_samples, refine_pri, regrid, regrid_doppler_frequencies)
from .pri_search import PriFold, describe_fold, find_pri, fold_z  # noqa: F401
from .pulse_doppler import PulseDoppler, detect_pulse_train, doppler_frequencies, range_doppler  # noqa: F401
from .pulse_mod import (MOP_DTYPE, PulseModulation, measure_pdws, measure_pulses, modulation_figures,  # noqa: F401
                        modulation_from_iq_file, phase_code, replica_from_measurement)
from .pulse_source import PulseTrain, pulse_train, synth_params  # noqa: F401
from .rd_cfar import RangeDopplerCfar, detect_maps, detect_targets  # noqa: F401
from .rd_cfar import detections_to_pdws as targets_to_pdws  # noqa: F401
from .stft import Stft, spectrogram_from_iq_file, stft, stft_axes  # noqa: F401
from .synthesizer import (ChannelSynthesizer, design_synthesis_taps, isolate_band, synthesis_delay,  # noqa: F401
                          synthesize)
from .trace import Envelope, Trace, envelope, envelope_from_iq_file  # noqa: F401
from .waterfall import Waterfall, WaterfallImage, waterfall, waterfall_from_iq_file  # noqa: F401

__all__ = ["Channelizer", "center_frequencies", "design_prototype", "pinned_empty", "PfbError", "LIB_PATH",
           "Stft", "stft", "stft_axes", "spectrogram_from_iq_file",
           "analyze_dwell", "dwell_from_iq_file", "fit_event", "next_event", "EventPredictor", "DwellStats",
           "PulseTrain", "pulse_train", "synth_params",
           "Trace", "Envelope", "envelope", "envelope_from_iq_file",
           "MatchedFilter", "compress", "compress_iq_file", "replica_from_pulse_train", "pulse_delay_from_iq_files",
           "Waterfall", "WaterfallImage", "waterfall", "waterfall_from_iq_file",
           "PulseClusterer", "cluster_pulses", "cluster_pdws", "cluster_items_from_pdws", "describe_clusterer",
           "deinterleave_clustered", "deinterleave_clustered_figures", "CLUSTER_ITEM_DTYPE", "CLUSTER_GROUP_DTYPE",
           "PulseAssociator", "associate", "associate_pdws", "fuse_pdws", "describe_associator", "ASSOC_ITEM_DTYPE",
           "GROUP_DTYPE",
           "ChannelSynthesizer", "synthesize", "design_synthesis_taps", "synthesis_delay", "isolate_band",
           "FinePriFold", "describe_fine_fold", "period_q32", "period_samples", "refine_pri", "find_pri_fine",
           "Regrid", "regrid", "regrid_doppler_frequencies", "detect_pulse_train_fine", "QSCORE_DTYPE",
           "MOP_DTYPE", "PulseModulation", "measure_pulses", "measure_pdws", "modulation_figures", "phase_code",
           "replica_from_measurement", "modulation_from_iq_file",
           "Deinterleaver", "deinterleave", "deinterleave_pdws", "deinterleave_detections", "merge_emitters",
           "describe_deinterleaver", "ticks_from_toa", "EMITTER_DTYPE",
           "OsCfar", "os_cfar_alpha", "detect_maps_os",
           "RangeDopplerCfar", "detect_maps", "detect_targets", "targets_to_pdws",
           "PriFold", "find_pri", "fold_z", "describe_fold",
           "PulseDoppler", "range_doppler", "doppler_frequencies", "detect_pulse_train",
           "Cfar", "cfar_alpha", "detect", "detect_pulses", "pulse_detections_from_iq_file", "detections_to_pdws",
           "MatchedFilterBank", "compress_bank", "bank_frequencies", "pulse_delay_and_offset_from_iq_files"]
