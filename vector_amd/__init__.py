"""vector_amd — MI355X-native DSP hot path of ramiyako/vector.

FIR -> decimate -> block FFT / PSD -> sliding cross-correlation, as hand-written
CDNA4 HIP kernels in libvsig.so (C ABI, include/vsig.h), behind the reference's
own Python call signatures (utils.py).  No CPU fallback: without the library or
a HIP device every call raises ``VsigUnavailable``.
"""
from ._lib import (RefineFault, VsigError, VsigInvalid, VsigUnavailable, get_context,  # noqa: F401
                   load_library)
from . import dsp  # noqa: F401
from .dsp import (Correlator, CorrelatorBank, FirFilter, FrequencySearch, Runs, SpectrumTraces,  # noqa: F401
                  find_runs,
                  averaged_spectrum, correlate, correlate_peak,
                  cross_correlate_signals, filter, find_correlation_peak,
                  find_packet_instances, find_packet_location_in_vector,
                  find_packet_location_with_offset, find_peaks, fir_filter, frequency_search,
                  peak_stats, spectrum)
from .spectrogram import create_spectrogram, spectrogram_params  # noqa: F401
from .channelizer import Channelizer, filter_channel, pfb_channelize  # noqa: F401
from .vectors import (apply_frequency_shift, resample_signal, load_packet, load_packet_info, mat2wv,  # noqa: F401
                      save_vector, save_vector_wv, transplant_packet_in_vector,
                      extract_reference_segment, measure_packet_timing, validate_transplant_quality,
                      transplant_and_validate,
                      VectorPlan, build_vector, compute_freq_ranges, validate_packet_timing, vector_plan,
                      verify_vector, extract_packets)
from .analysis import (Packets, boxcar_energy, detect_packet_bounds, detect_packets, find_packet_start,  # noqa: F401
                       normalize_spectrogram, order_statistics, threshold_stats)
from .display import (SpectrogramImage, colormap_table, image_extent, plot_spectrogram_image,  # noqa: F401
                      pool_factors, spectrogram_image, spectrogram_levels)
from .traces import Trace, averaged_spectrum_trace, capture_spectrum, signal_envelope, trace_bin  # noqa: F401
from .packets import (IsolatedPackets, PacketMeasurements, SegmentSpectra, design_lowpass,  # noqa: F401
                      isolate_packets, measure_packets, segment_spectra)
from .match import (CombinedPackets, CombineMembers, GroupTiming, PacketGroups, PacketMatches,  # noqa: F401
                    Similarity, cluster_carriers, combine_packets, group_packets, group_timing, match_packets,
                    packet_similarity)

__version__ = "0.1.0"
