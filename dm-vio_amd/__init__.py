"""dm-vio_amd — MI355X-native photometric direct alignment (DM-VIO hot path).

This Python package is only the test/bench harness side of the C ABI in include/dmvio_hip.h
(ctypes over dm-vio_amd/lib/libdmvio_hip.so).  The product is the shared library; there is NO
CPU fallback: if the HIP library is missing or no GPU is visible, every compute entry raises.

_abi.py declares the ABI (one signature table, the struct mirrors, the loader, the handle base); the wrappers sit in one
module per unit of the library (frames, tracker, initializer, points, ba) and are re-exported here.

The directory name contains a hyphen (it mirrors the reference's name), so import it through
`__graft_entry__.load_package()` / tests/conftest.py, which register it as module `dmvio_amd`.
"""
from ._abi import (INCLUDE_PATH, LIB_PATH, MIRRORS, SIGNATURES, ActivationOptimize, ActivationWindow, BACallbacks, BAFrameView, BAGraphWindow, BAMargFrameWindow,  # noqa: F401
                   BAMargWindow, BAVioOptions, CoarseCallbacks, CommCallbacks, HipLibraryError, InitializerPointsWindow, InitializerWindow, NewTracesWindow,
                   PixelSelectorSettings, PixelSelectorWindow, SetRefBaWindow, SetRefWindow, TraceTablesWindow, TraceWindow, TrackerSettings, _ALLGATHER, _ALLREDUCE_F64, _chk, _d, _err, _f, _i,
                   c_d, c_f, c_i, c_u8, declared_symbols, load_library)
from .frames import Context, UndistorterHip, frame_level0_is_tiled, set_raw_batch_kernel, set_raw_batch_layout  # noqa: F401
from .tracker import CoarseTrackerHip, SetRefBatchHip, TrackMultiHip, coarse_update_visual, make_track_hypotheses, write_result_txt  # noqa: F401
from .initializer import CoarseInitializerHip, InitFirstHip, InitializerBatchHip  # noqa: F401
from .points import (STATUS_NAMES, ActivationBatchHip, DistanceMapHip, ImmaturePointsHip, PixelSelectorBatchHip, PixelSelectorHip, TraceBatchHip, activate_points,  # noqa: F401
                     activate_points_batch, distance_map_tables, min_act_dist_update)
from .ba import BundleAdjusterBatch, BundleAdjusterHip, RcclCommunicator, WindowGraph, debug_solve, host_solve_ldlt  # noqa: F401
