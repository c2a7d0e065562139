"""ctypes binding of libralign_hip.so (include/ralign.h).

Mirrors the reference's ctypes boundary (test_mref_gpu_align.py:91-149: cu_module,
AlignConfig, AlignParam, get_c_ptr_array) and adds the handle-based ra_* API that works
on device pointers (torch CUDA tensors supply the memory and the stream).

There is no CPU fallback: if the HIP library is missing or fails to load, importing the
engine raises.
"""
import ctypes
import os

import numpy as np

from ._common import Launcher, ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RALIGN_LIB") or os.path.join(_HERE, "libralign_hip.so")   # RALIGN_LIB: another build of the same library (kernel experiments)

RA_MODE_MREF = 0
RA_MODE_REFFREE = 1
RA_INTERP_BILINEAR = 0      # Util::bilinear in alrl_ms (EMAN2 2.31; default)
RA_INTERP_QUADRI = 1        # Util::quadri (older releases): size-generic kernels


class AlignConfig(ctypes.Structure):
    # reference: test_mref_gpu_align.py:112-123 / cuda/gpu_aln_common.h:62-74
    _fields_ = [("sbj_num", ctypes.c_uint), ("ref_num", ctypes.c_uint), ("img_dim", ctypes.c_uint),
                ("ring_num", ctypes.c_uint), ("ring_len", ctypes.c_uint),
                ("shift_step", ctypes.c_float), ("shift_rng_x", ctypes.c_float), ("shift_rng_y", ctypes.c_float)]


class AlignParam(ctypes.Structure):
    # reference: test_mref_gpu_align.py:125-134 / cuda/gpu_aln_common.h:76-83
    _fields_ = [("sbj_id", ctypes.c_int), ("ref_id", ctypes.c_int), ("shift_x", ctypes.c_float),
                ("shift_y", ctypes.c_float), ("angle", ctypes.c_float), ("mirror", ctypes.c_bool)]

    def __str__(self):
        return "s_%d/r_%d::(%d,%d;%.2f)" % (self.sbj_id, self.ref_id, self.shift_x, self.shift_y, self.angle) \
            + ("[M]" if self.mirror else "")


class RaConfig(ctypes.Structure):
    _fields_ = [("nx", ctypes.c_int), ("first_ring", ctypes.c_int), ("last_ring", ctypes.c_int),
                ("ring_skip", ctypes.c_int), ("xrng", ctypes.c_float), ("yrng", ctypes.c_float),
                ("step", ctypes.c_float), ("nref", ctypes.c_int), ("mode", ctypes.c_int),
                ("device", ctypes.c_int), ("chunk", ctypes.c_int)]


class RaOptions(ctypes.Structure):
    # include/ralign.h: ra_options
    _fields_ = [("interp", ctypes.c_int), ("normalize_ring", ctypes.c_int)]


# ra_result as a numpy record (32 bytes)
RESULT_DTYPE = np.dtype([("alpha", np.float32), ("sx", np.float32), ("sy", np.float32), ("mirror", np.int32),
                         ("ref_id", np.int32), ("peak", np.float32), ("angle_bin", np.int32),
                         ("shift_idx", np.int32)])
# candidate record of the search kernels (CandT, 40 bytes): peak, jtot word (bits 0-12 jtot | 13-20 runner-up reference + 1 | 21 its
# mirror flag | 22-31 its jtot), reference | mirror << 16, the 7 CCF samples around the peak
CAND_DTYPE = np.dtype([("val", np.float32), ("jtot", np.int32), ("refmir", np.int32), ("t7", np.float32, (7,))])
# record of the refine list (RefineRec, 120 bytes): the winner and up to 7 alternates (offset, reference tile, reference | mirror << 16)
REFINE_ALTS = 7
REFINE_DTYPE = np.dtype([("p", np.int32), ("ref", np.int32), ("mirror", np.int32), ("jtot", np.int32), ("bs", np.int32),
                         ("brt", np.int32), ("sxi", np.float32), ("syi", np.float32), ("nalt", np.int32),
                         ("alt", np.dtype([("bs", np.int32), ("rt", np.int32), ("refmir", np.int32)]), (REFINE_ALTS,))])
assert CAND_DTYPE.itemsize == 40 and REFINE_DTYPE.itemsize == 120 and REFINE_DTYPE.fields["alt"][1] == 36


class RaLdsRow(ctypes.Structure):
    _fields_ = [("kernel", ctypes.c_char * 64), ("static_bytes", ctypes.c_int), ("dynamic_bytes", ctypes.c_int),
                ("limit_bytes", ctypes.c_int)]


float_ptr = ctypes.POINTER(ctypes.c_float)
aln_param_ptr = ctypes.POINTER(AlignParam)

# every symbol include/ralign.h declares
EXPORTED_SYMBOLS = [
    "print_gpu_info", "gpu_clear", "pre_align_init", "pre_align_size_check", "pre_align_fetch",
    "pre_align_run", "pre_align_run_m", "mref_align_run", "mref_align_run_m", "get_num_ref", "reset_shifts",
    "ref_free_alignment_2D_init", "ref_free_alignment_2D_size_check", "ref_free_alignment_2D",
    "ref_free_alignment_2D_filter_references", "ra_isac_get_references", "ra_legacy_bytes",
    "ra_last_error", "ra_create", "ra_destroy", "ra_set_stream", "ra_num_shifts", "ra_maxrin", "ra_lcirc", "ra_search_path", "ra_search_tiled", "ra_search_l1_tap_rings", "ra_l1_tap_rule", "ra_search_offsets_per_pass", "ra_set_nomirror", "ra_set_mask",
    "ra_reset_shifts", "ra_set_references", "ra_get_prepared_references", "ra_align", "ra_state_from_params", "ra_set_refine", "ra_set_class_references", "ra_align_classes",
    "ra_debug_spectra", "ra_debug_exact_references", "ra_debug_finalize", "ra_debug_refine", "ra_transform_accumulate", "ra_update_references", "ra_normalize_particles", "ra_sync", "ra_kernel_time",
    "ra_fsc_len", "ra_class_fsc", "ra_last_class_fsc", "ra_fit_tanh", "ra_class_averages", "ra_filter_references",
    "ra_state_from_params_dev", "ra_class_fsc_fit", "ra_filter_references_dev", "ra_last_refine_count", "ra_lds_report",
    "ra_create_ex", "ra_set_normalize_ring", "ra_get_options", "ra_search_skips_offsets", "ra_phase_flip",
    "ra_sdr_mean", "ra_sdr_gram", "ra_sdr_project", "ra_sdr_factors", "ra_rot_shift2d", "ra_sdr_reconstruct",
    "ra_tsne_knn", "ra_tsne_affinity", "ra_tsne_step", "ra_tsne_error",
    "ra_tsne_knn_query", "ra_tsne_affinity_rows", "ra_tsne_place_gradient", "ra_tsne_place",
    "ra_kmeans_sqnorm", "ra_kmeans_labels", "ra_kmeans_lloyd", "ra_kmeans_search", "ra_kmeans_seed",
    "ra_kmeans_silhouette", "ra_kmeans_dispersion", "ra_gmm_estep", "ra_gmm_mstep", "ra_dbscan_count", "ra_dbscan_step",
    "ra_hdbscan_core", "ra_hdbscan_round", "ra_ward_nearest", "ra_ward_merge", "ra_embed_ranks",
    "ra_spectral_spmv", "ra_spectral_lanczos", "ra_spectral_ritz", "ra_spectral_components", "ra_spectral_work_bytes",
    "ra_umap_smooth_knn", "ra_umap_epochs", "ra_umap_place",
    "ra_fourier_resize", "ra_wiener_accumulate", "ra_wiener_finalize", "ra_wiener_frc", "ra_wiener_finalize_ssnr", "ra_wiener_score",
    "ra_prep_normalize", "ra_prep_filter",
]

_lib = None


class EngineError(RuntimeError):
    pass


def load_library(path=None):
    """dlopen libralign_hip.so and declare prototypes.  Raises if the library is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    # torch bundles its own HIP runtime (libamdhip64.so.7); it must be the one already mapped when
    # this library is opened, otherwise the process ends up with two runtimes and no device
    import torch  # noqa: F401
    if not os.path.exists(p):
        raise EngineError("HIP alignment library not built: %s (run `python -m cryo_ralib_amd.build`)" % p)
    L = ctypes.CDLL(p)
    vp = ctypes.c_void_p
    L.ra_last_error.restype = ctypes.c_char_p
    L.ra_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(RaConfig)]
    L.ra_create_ex.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(RaConfig), ctypes.POINTER(RaOptions)]
    L.ra_set_normalize_ring.argtypes = [vp, ctypes.c_int]
    L.ra_get_options.argtypes = [vp, ctypes.POINTER(RaOptions)]
    L.ra_destroy.argtypes = [vp]
    L.ra_destroy.restype = None
    L.ra_set_stream.argtypes = [vp, vp]
    L.ra_num_shifts.argtypes = [vp]
    L.ra_maxrin.argtypes = [vp]
    L.ra_lcirc.argtypes = [vp]
    L.ra_search_path.argtypes = [vp]
    L.ra_search_tiled.argtypes = [vp]
    if hasattr(L, "ra_search_l1_tap_rings"):      # (an older build loaded through RALIGN_LIB for a side-by-side measurement has none)
        L.ra_search_l1_tap_rings.argtypes = [vp]
        L.ra_l1_tap_rule.argtypes = [ctypes.c_int] * 4 + [ctypes.c_float] * 2
    L.ra_search_skips_offsets.argtypes = [vp]
    L.ra_search_offsets_per_pass.argtypes = [vp]
    L.ra_set_nomirror.argtypes = [vp, ctypes.c_int]
    L.ra_set_mask.argtypes = [vp, vp]
    L.ra_reset_shifts.argtypes = [vp, ctypes.c_float, ctypes.c_float, ctypes.c_float]
    L.ra_set_references.argtypes = [vp, vp]
    L.ra_get_prepared_references.argtypes = [vp, vp]
    L.ra_align.argtypes = [vp, vp, ctypes.c_int, vp, vp, float_ptr]
    L.ra_set_class_references.argtypes = [vp, vp, ctypes.c_int]
    L.ra_align_classes.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp]
    L.ra_state_from_params.argtypes = [vp, vp, ctypes.c_int, float_ptr, vp]
    L.ra_set_refine.argtypes = [vp, ctypes.c_float]
    L.ra_last_refine_count.argtypes = [vp]
    L.ra_lds_report.argtypes = [vp, ctypes.POINTER(RaLdsRow), ctypes.c_int]
    L.ra_state_from_params_dev.argtypes = [vp, vp, ctypes.c_int, vp, vp]
    L.ra_class_fsc_fit.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, vp, vp]
    L.ra_filter_references_dev.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, vp]
    L.ra_transform_accumulate.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    L.ra_update_references.argtypes = [vp, vp, vp, ctypes.c_int, vp]
    L.ra_normalize_particles.argtypes = [vp, vp, ctypes.c_int]
    L.ra_sync.argtypes = [vp]
    L.ra_debug_spectra.argtypes = [vp, vp, ctypes.c_int, vp, vp]
    L.ra_debug_exact_references.argtypes = [vp, vp, vp]
    L.ra_debug_finalize.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, vp, vp, vp,
                                    ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.ra_debug_refine.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, vp, vp]
    L.ra_kernel_time.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                 ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    L.ra_fsc_len.argtypes = [vp]
    L.ra_class_fsc.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, float_ptr]
    L.ra_last_class_fsc.argtypes = [vp, float_ptr]
    L.ra_fit_tanh.argtypes = [float_ptr, float_ptr, ctypes.c_int, float_ptr, float_ptr]
    L.ra_class_averages.argtypes = [vp, vp, vp, ctypes.c_int, vp]
    L.ra_filter_references.argtypes = [vp, vp, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int, float_ptr,
                                       ctypes.c_int, float_ptr]
    # reference surface (test_mref_gpu_align.py:95-97 sets the pointer returns to c_ulonglong)
    L.pre_align_init.restype = ctypes.c_ulonglong
    L.pre_align_init.argtypes = [ctypes.c_uint, ctypes.POINTER(AlignConfig), ctypes.c_uint]
    L.pre_align_size_check.restype = ctypes.c_bool
    L.pre_align_size_check.argtypes = [ctypes.c_uint, ctypes.POINTER(AlignConfig), ctypes.c_uint, ctypes.c_float,
                                       ctypes.c_bool]
    L.pre_align_fetch.argtypes = [ctypes.POINTER(float_ptr), ctypes.c_uint, ctypes.c_char_p]
    L.pre_align_fetch.restype = None
    L.pre_align_run.argtypes = [ctypes.c_int, ctypes.c_int]
    L.pre_align_run.restype = None
    L.pre_align_run_m.argtypes = [ctypes.c_int, ctypes.c_int]
    L.pre_align_run_m.restype = ctypes.c_ulonglong
    L.mref_align_run.argtypes = [ctypes.c_int, ctypes.c_int]
    L.mref_align_run.restype = ctypes.c_ulonglong
    L.mref_align_run_m.argtypes = [ctypes.c_int, ctypes.c_int]
    L.mref_align_run_m.restype = float_ptr
    L.get_num_ref.restype = ctypes.POINTER(ctypes.c_int)
    L.reset_shifts.argtypes = [ctypes.c_float, ctypes.c_float]
    L.reset_shifts.restype = None
    L.print_gpu_info.argtypes = [ctypes.c_uint]
    L.print_gpu_info.restype = None
    L.gpu_clear.restype = None
    L.ref_free_alignment_2D_init.restype = ctypes.c_ulonglong
    L.ref_free_alignment_2D_init.argtypes = [ctypes.POINTER(AlignConfig), ctypes.POINTER(float_ptr), ctypes.POINTER(float_ptr),
                                             ctypes.POINTER(ctypes.c_int), ctypes.c_uint]
    L.ref_free_alignment_2D_size_check.restype = ctypes.c_bool
    L.ref_free_alignment_2D_size_check.argtypes = [ctypes.POINTER(AlignConfig), ctypes.c_uint, ctypes.c_float, ctypes.c_bool]
    L.ref_free_alignment_2D.restype = None
    L.ref_free_alignment_2D.argtypes = []
    L.ref_free_alignment_2D_filter_references.restype = None
    L.ref_free_alignment_2D_filter_references.argtypes = [ctypes.c_float, ctypes.c_float]
    L.ra_isac_get_references.argtypes = [float_ptr]
    L.ra_phase_flip.argtypes = [vp, ctypes.c_int, ctypes.c_int, float_ptr, ctypes.c_int, vp]
    ci = ctypes.c_int
    L.ra_fourier_resize.argtypes = [vp, ci, ci, ci, vp, vp]
    L.ra_wiener_accumulate.argtypes = [vp, ci, ci, vp, float_ptr, ci, ci, ci, vp, vp, vp, vp]
    L.ra_wiener_finalize.argtypes = [vp, vp, vp, ci, ci, ci, ctypes.c_float, ci, vp, vp]
    L.ra_wiener_frc.argtypes = [vp, vp, vp, ci, ci, ci, ctypes.c_float, ci, ctypes.c_float, vp, vp, vp]
    L.ra_wiener_finalize_ssnr.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp, vp]
    L.ra_wiener_score.argtypes = [vp, ci, ci, vp, float_ptr, ci, ci, ci, vp, vp, vp, ctypes.c_float, vp, ci, ci, ci, vp, vp]
    L.ra_prep_normalize.argtypes = [vp, ci, ci, ctypes.c_double, ci, ci, vp, vp]
    L.ra_prep_filter.argtypes = [vp, ci, ci, ci, ci, ctypes.c_double, ctypes.c_double, ci, ctypes.c_double, ctypes.c_double, vp]
    L.ra_sdr_mean.argtypes = [vp, ci, ci, ci, vp, vp]
    L.ra_sdr_gram.argtypes = [vp, ci, ci, ci, vp, ci, vp, ci, vp, vp]
    L.ra_sdr_project.argtypes = [vp, ci, ci, ci, vp, vp, ci, vp, ci, vp, vp]
    L.ra_sdr_factors.argtypes = [vp, ci, ci, vp, ci, vp, vp]
    L.ra_rot_shift2d.argtypes = [vp, ci, ci, vp, vp, vp]
    L.ra_sdr_reconstruct.argtypes = [vp, ci, ci, vp, ci, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp]
    cf = ctypes.c_float
    L.ra_tsne_knn.argtypes = [vp, ci, ci, ci, vp, vp, vp]
    L.ra_tsne_affinity.argtypes = [vp, ci, ci, cf, vp, vp]
    L.ra_tsne_step.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, ci, cf, cf, cf, vp, vp]
    L.ra_tsne_error.argtypes = [vp, ci, vp, vp, vp, ci, cf, vp, vp, vp]
    L.ra_tsne_knn_query.argtypes = [vp, ci, vp, ci, ci, ci, vp, vp, vp]
    L.ra_tsne_affinity_rows.argtypes = [vp, ci, ci, cf, vp, vp]
    L.ra_tsne_place_gradient.argtypes = [vp, ci, vp, ci, vp, vp, ci, cf, vp, vp, vp, vp]
    L.ra_tsne_place.argtypes = [vp, ci, vp, ci, vp, vp, ci, cf, cf, cf, ci, vp, vp]
    L.ra_kmeans_sqnorm.argtypes = [vp, ci, ci, vp, vp]
    L.ra_kmeans_labels.argtypes = [vp, ci, ci, vp, vp, ci, vp, ci, vp, vp]
    L.ra_kmeans_lloyd.argtypes = [vp, ci, ci, vp, vp, ci, vp, vp, vp, vp]
    L.ra_kmeans_search.argtypes = [vp, ci, vp, ci, vp, vp]
    L.ra_kmeans_seed.argtypes = [vp, ci, ci, vp, ci, vp, ci, vp, vp]
    L.ra_kmeans_silhouette.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp]
    L.ra_kmeans_dispersion.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp, vp, vp]
    L.ra_gmm_estep.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ra_gmm_mstep.argtypes = [vp, ci, ci, ci, ci, vp, ci, ctypes.c_double, vp, vp, vp, vp]
    L.ra_dbscan_count.argtypes = [vp, ci, ci, ctypes.c_double, ci, vp, vp, vp]
    L.ra_dbscan_step.argtypes = [vp, ci, ci, ctypes.c_double, vp, ci, vp, vp, vp, vp]
    L.ra_hdbscan_core.argtypes = [vp, ci, ci, ci, vp, vp]
    L.ra_hdbscan_round.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp]
    L.ra_ward_nearest.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, vp]
    L.ra_ward_merge.argtypes = [vp, vp, ci, ci, vp, vp, ci, vp]
    L.ra_embed_ranks.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp]
    L.ra_spectral_spmv.argtypes = [vp, vp, vp, ci, vp, vp, vp]
    L.ra_spectral_lanczos.argtypes = [vp, vp, vp, ci, vp, vp, ci, ci, ci, vp, vp, vp, vp]
    L.ra_spectral_ritz.argtypes = [vp, ci, ci, ci, vp, ci, vp, vp]
    L.ra_spectral_components.argtypes = [vp, vp, ci, vp, vp, vp]
    L.ra_spectral_work_bytes.restype = ctypes.c_size_t
    L.ra_spectral_work_bytes.argtypes = [ci, ci]
    cd, cu64 = ctypes.c_double, ctypes.c_uint64
    L.ra_umap_smooth_knn.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp]
    L.ra_umap_epochs.argtypes = [vp, vp, ci, vp, vp, vp, ci, cd, cd, cd, ci, cd, ci, ci, ci, cu64, vp]
    L.ra_umap_place.argtypes = [vp, ci, ctypes.c_longlong, vp, ci, vp, vp, ci, cd, cd, cd, ci, cd, ci, cu64, vp]
    L.ra_legacy_bytes.restype = ctypes.c_size_t
    L.ra_legacy_bytes.argtypes = [ctypes.c_uint, ctypes.POINTER(AlignConfig)]
    if path is None:
        _lib = L
    return L


def get_c_ptr_array(images):
    """array of float* over C-contiguous float32 images (test_mref_gpu_align.py:138-146)."""
    ptrs = []
    for img in images:
        assert img.flags["C_CONTIGUOUS"] and img.dtype == np.float32
        ptrs.append(img.ctypes.data_as(float_ptr))
    return (float_ptr * len(ptrs))(*ptrs)


def fit_tanh(dres, low=0.1):
    """sp_filter.fit_tanh on an fsc result [freq, fsc, n]; edits dres[1] in place like the original"""
    assert low == 0.1
    n = len(dres[0])
    fr = (ctypes.c_float * n)(*dres[0])
    fs = (ctypes.c_float * n)(*dres[1])
    fl, aa = ctypes.c_float(), ctypes.c_float()
    _check(load_library().ra_fit_tanh(fr, fs, n, ctypes.byref(fl), ctypes.byref(aa)), "ra_fit_tanh")
    dres[1][:] = [float(v) for v in fs]
    return fl.value, aa.value


def phase_flip(images, ctf, pad=True):
    """CTF phase flip of images [n][nx][nx] (contiguous float32 CUDA tensor), in place, on the current stream (ra_phase_flip).
    ctf: [n][9] table in the utils_ralib.parse_ctf_star layout (numpy or tensor; it is checked on the host before the launch).
    pad=True embeds every image in a 2nx x 2nx zero image (SPHIRE filt_ctf's default padding), pad=False flips at nx.
    Returns `images`."""
    import torch
    assert images.is_cuda and images.is_contiguous() and images.dtype == torch.float32, "images: contiguous float32 CUDA tensor"
    assert images.dim() == 3 and images.shape[1] == images.shape[2], "images: [n][nx][nx]"
    n, nx = int(images.shape[0]), int(images.shape[-1])
    if isinstance(ctf, torch.Tensor):
        ctf = ctf.detach().cpu().numpy()
    tab = np.ascontiguousarray(ctf, np.float32)
    if tab.shape != (n, 9):
        raise EngineError("phase_flip: the CTF table is [%d][9], got %s" % (n, tab.shape))
    L = Launcher(images)
    with torch.cuda.device(images.device):
        L.call("ra_phase_flip", ptr(images), n, nx, tab.ctypes.data_as(float_ptr), int(bool(pad)))
    return images


def rot_shift2d(images, params, out=None):
    """rot_shift2D of images [n][nx][nx] (contiguous float32 CUDA tensor) by params [n][4] (alpha, sx, sy, mirror), on the current
    stream (ra_rot_shift2d): the transform of Engine.transform_accumulate, without an engine. Returns out ([n][nx][nx])."""
    import torch
    assert images.is_cuda and images.is_contiguous() and images.dtype == torch.float32, "images: contiguous float32 CUDA tensor"
    assert images.dim() == 3 and images.shape[1] == images.shape[2], "images: [n][nx][nx]"
    n, nx = int(images.shape[0]), int(images.shape[-1])
    if isinstance(params, torch.Tensor):
        params = params.detach().cpu().numpy()
    prm = np.asarray(params, np.float64)
    if prm.shape != (n, 4):
        raise EngineError("rot_shift2d: params is [%d][4] (alpha, sx, sy, mirror), got %s" % (n, prm.shape))
    rec = np.zeros(n, RESULT_DTYPE)
    rec["alpha"], rec["sx"], rec["sy"] = prm[:, 0], prm[:, 1], prm[:, 2]
    rec["mirror"] = (prm[:, 3] != 0).astype(np.int32)
    if out is None:
        out = torch.empty_like(images)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.shape == images.shape, "out: like images"
    d_rec = torch.from_numpy(rec.view(np.uint8)).to(images.device)
    L = Launcher(images)
    with torch.cuda.device(images.device):
        L.call("ra_rot_shift2d", ptr(images), n, nx, ptr(d_rec), ptr(out))
    return out


def fourier_resize(images, m, out=None):
    """Fourier resizing of images [n][nx][nx] (contiguous float32 CUDA tensor) to [n][m][m], on the current stream
    (ra_fourier_resize): y = A x A^T with resize.operator(nx, m); 1 <= nx, m <= 1024.  out: a contiguous float32 [n][m][m] tensor
    on the same device that does not overlap images, or None (allocated).  Returns out."""
    import torch
    assert images.is_cuda and images.is_contiguous() and images.dtype == torch.float32, "images: contiguous float32 CUDA tensor"
    assert images.dim() == 3 and images.shape[1] == images.shape[2], "images: [n][nx][nx]"
    n, nx, m = int(images.shape[0]), int(images.shape[-1]), int(m)
    if out is None:
        if not 1 <= m <= 1024:
            raise EngineError("fourier_resize: need 1 <= m <= 1024, got %d" % m)
        out = torch.empty((n, m, m), dtype=torch.float32, device=images.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.device == images.device \
        and tuple(out.shape) == (n, m, m), "out: contiguous float32 [n][m][m] on the images' device"
    L = Launcher(images)
    with torch.cuda.device(images.device):
        L.call("ra_fourier_resize", ptr(images), n, nx, m, ptr(out))
    return out


def normalize_background(images, bg_radius, **kw):
    """Background normalisation of a stack, with optional plane removal and contrast inversion (prep.normalize)."""
    from . import prep
    return prep.normalize(images, bg_radius, **kw)


def fourier_filter(images, **kw):
    """Low-pass / high-pass / band-pass Fourier filter of a stack (prep.fourier_filter)."""
    from . import prep
    return prep.fourier_filter(images, **kw)


def wiener_averages(images, params, labels, k, ctf, **kw):
    """CTF-corrected (Wiener) class averages [k][nx][nx] and class sizes of an aligned stack (wiener.wiener_averages)."""
    from . import wiener
    return wiener.wiener_averages(images, params, labels, k, ctf, **kw)


def ssnr_averages(images, params, labels, k, ctf, **kw):
    """SSNR-weighted Wiener class averages [k][nx][nx], class sizes, half-set FRC curves [k][P/2 + 1] and resolutions
    (wiener.ssnr_averages)."""
    from . import wiener
    return wiener.ssnr_averages(images, params, labels, k, ctf, **kw)


def particle_scores(images, params, labels, k, ctf, **kw):
    """Per-particle agreement with the class's Wiener estimate, leave-one-out by default: ({"cc", "scale", "sums"}, class sizes)
    (wiener.particle_scores; wiener.select turns cc into a mask of the particles to keep)."""
    from . import wiener
    return wiener.particle_scores(images, params, labels, k, ctf, **kw)


def two_sdr(images, p0, q0, r, **kw):
    """Two-stage dimension reduction of images [n][p][q] (sdr.two_sdr)."""
    from . import sdr
    return sdr.two_sdr(images, p0, q0, r, **kw)


def mpca(images, p0, q0, **kw):
    """MPCA of images [n][p][q] (sdr.mpca)."""
    from . import sdr
    return sdr.mpca(images, p0, q0, **kw)


def sdr_transform(images, model, **kw):
    """Factors [n][r] of images [n][p][q] under a fitted sdr.SdrModel (sdr.transform)."""
    from . import sdr
    return sdr.transform(images, model, **kw)


def sdr_reconstruct(factors, model, **kw):
    """Images [n][p][q] rebuilt from factors [n][r] under a fitted sdr.SdrModel (sdr.reconstruct)."""
    from . import sdr
    return sdr.reconstruct(factors, model, **kw)


def sdr_denoise(images, model, **kw):
    """reconstruct(transform(images)), with residuals=True also |x - x^|^2 per image (sdr.denoise)."""
    from . import sdr
    return sdr.denoise(images, model, **kw)


def tsne(X, **kw):
    """t-SNE embedding [n][2] of X [n][d] (tsne.tsne)."""
    from . import tsne as _tsne
    return _tsne.tsne(X, **kw)


def tsne_transform(X_new, X_fit, Y_fit, **kw):
    """New rows placed into a fitted embedding: [n][2] float32 (tsne.transform)."""
    from . import tsne as _tsne
    return _tsne.transform(X_new, X_fit, Y_fit, **kw)


def tsne_knn_query(Q, X, k, **kw):
    """(idx [nq][k], dist2 [nq][k]) of the k rows of X nearest every row of Q (tsne.knn_query)."""
    from . import tsne as _tsne
    return _tsne.knn_query(Q, X, k, **kw)


def tsne_vote_labels(idx, p, labels_fit):
    """(labels, confidence) of placed rows by the neighbour vote over the fitted rows' labels (tsne.vote_labels)."""
    from . import tsne as _tsne
    return _tsne.vote_labels(idx, p, labels_fit)


def tsne_large(X, fit_size, **kw):
    """t-SNE of up to 4194304 rows: a fit on fit_size drawn rows, the rest placed into it (tsne.tsne_large)."""
    from . import tsne as _tsne
    return _tsne.tsne_large(X, fit_size, **kw)


def kmeans(X, n_clusters, **kw):
    """k-means of X [n][d] (kmeans.kmeans): KMeansResult with labels, centers, inertia, n_iter, init_indices."""
    from . import kmeans as _kmeans
    return _kmeans.kmeans(X, n_clusters, **kw)


def silhouette_samples(X, labels, **kw):
    """Silhouette coefficient of every sample, float64 [n] (kmeans.silhouette_samples)."""
    from . import kmeans as _kmeans
    return _kmeans.silhouette_samples(X, labels, **kw)


def silhouette_score(X, labels, **kw):
    """Mean silhouette coefficient, optionally of sklearn's subsample (kmeans.silhouette_score)."""
    from . import kmeans as _kmeans
    return _kmeans.silhouette_score(X, labels, **kw)


def calinski_harabasz_score(X, labels, **kw):
    """Calinski-Harabasz index (kmeans.calinski_harabasz_score)."""
    from . import kmeans as _kmeans
    return _kmeans.calinski_harabasz_score(X, labels, **kw)


def davies_bouldin_score(X, labels, **kw):
    """Davies-Bouldin index (kmeans.davies_bouldin_score)."""
    from . import kmeans as _kmeans
    return _kmeans.davies_bouldin_score(X, labels, **kw)


def validity(X, labels, **kw):
    """Silhouette (overall and per class), Calinski-Harabasz, Davies-Bouldin and cluster sizes (kmeans.validity)."""
    from . import kmeans as _kmeans
    return _kmeans.validity(X, labels, **kw)


def kmeans_sweep(X, ks, **kw):
    """k-means and the validity scores for every k of ks on one device copy of X (kmeans.sweep)."""
    from . import kmeans as _kmeans
    return _kmeans.sweep(X, ks, **kw)


def gmm(X, n_components, **kw):
    """Gaussian mixture of X [n][d] (gmm.gmm): GmmResult with weights, means, covariances, precisions_cholesky, labels, ..."""
    from . import gmm as _gmm
    return _gmm.gmm(X, n_components, **kw)


def gmm_predict_proba(X, model, **kw):
    """Posterior probabilities [n][k] of a fitted mixture (gmm.predict_proba)."""
    from . import gmm as _gmm
    return _gmm.predict_proba(X, model, **kw)


def gmm_sweep(X, ks, **kw):
    """A mixture and its BIC / AIC for every k of ks on one device copy of X (gmm.sweep)."""
    from . import gmm as _gmm
    return _gmm.sweep(X, ks, **kw)


def dbscan(X, eps, **kw):
    """DBSCAN of X [n][d] (dbscan.dbscan): DbscanResult with labels (-1 for noise), core_mask, core_sample_indices, n_clusters, ..."""
    from . import dbscan as _dbscan
    return _dbscan.dbscan(X, eps, **kw)


def hdbscan(X, **kw):
    """HDBSCAN of X [n][d] (hdbscan.hdbscan): HdbscanResult with labels (-1 for noise), probabilities, tie_mask, n_clusters, ..."""
    from . import hdbscan as _hdbscan
    return _hdbscan.hdbscan(X, **kw)


def ward(X, **kw):
    """Ward clustering of X [n][d] (ward.ward): WardResult with labels, n_clusters, counts, centers and the tree."""
    from . import ward as _ward
    return _ward.ward(X, **kw)


def ward_linkage(X, **kw):
    """The Ward dendrogram of X [n][d] (ward.linkage): WardTree with Z (scipy's layout), children, heights, w2, n_rounds, ..."""
    from . import ward as _ward
    return _ward.linkage(X, **kw)


def ward_cut(tree, **kw):
    """int32 [n] labels of a WardTree cut at n_clusters or at distance_threshold (ward.cut)."""
    from . import ward as _ward
    return _ward.cut(tree, **kw)


def ward_sweep(X, ks, **kw):
    """One Ward tree, then its cut, inertia and the validity scores for every k of ks (ward.sweep)."""
    from . import ward as _ward
    return _ward.sweep(X, ks, **kw)


def spectral_embedding(X, **kw):
    """Spectral embedding (diffusion map) of X [n][d] (spectral.embedding): SpectralResult with embedding, eigenvalues, residuals, ..."""
    from . import spectral as _spectral
    return _spectral.embedding(X, **kw)


def spectral_cluster(X, n_clusters, **kw):
    """Spectral clustering of X [n][d] (spectral.cluster): labels (-1 outside the embedded component), the embedding and the k-means result."""
    from . import spectral as _spectral
    return _spectral.cluster(X, n_clusters, **kw)


def spectral_graph(X, **kw):
    """The symmetric kNN graph of X [n][d] (spectral.graph): (indptr, indices, a, component)."""
    from . import spectral as _spectral
    return _spectral.graph(X, **kw)


def umap(X, **kw):
    """UMAP embedding of X [n][d] (umap.umap): UmapResult with embedding [n][2], graph, a, b, n_epochs, init."""
    from . import umap as _umap
    return _umap.umap(X, **kw)


def umap_transform(X_new, X_fit, Y_fit, **kw):
    """Place X_new into the UMAP embedding Y_fit of X_fit (umap.transform)."""
    from . import umap as _umap
    return _umap.transform(X_new, X_fit, Y_fit, **kw)


def umap_fuzzy_graph(X, **kw):
    """The fuzzy simplicial set of X [n][d] (umap.fuzzy_graph): (indptr, indices, s, rho, sigma)."""
    from . import umap as _umap
    return _umap.fuzzy_graph(X, **kw)


def dbscan_kdistances(X, min_samples, **kw):
    """For every point the least eps at which it is a core point, float64 [n] (dbscan.kdistances)."""
    from . import dbscan as _dbscan
    return _dbscan.kdistances(X, min_samples, **kw)


def trustworthiness(X, Y, **kw):
    """Trustworthiness of the embedding Y of X (quality.trustworthiness): do the neighbours in Y lie near in X?"""
    from . import quality as _quality
    return _quality.trustworthiness(X, Y, **kw)


def continuity(X, Y, **kw):
    """Continuity of the embedding Y of X (quality.continuity): do the neighbours in X stay near in Y?"""
    from . import quality as _quality
    return _quality.continuity(X, Y, **kw)


def embedding_quality(X, Y, **kw):
    """Trustworthiness, continuity, their per-point scores and the co-ranking curve in one call (quality.embedding_quality)."""
    from . import quality as _quality
    return _quality.embedding_quality(X, Y, **kw)


def neighbor_ranks(A, idx, **kw):
    """int32 [n][k]: the rank in A's row i of every entry of the lists idx [n][k] (quality.neighbor_ranks)."""
    from . import quality as _quality
    return _quality.neighbor_ranks(A, idx, **kw)


def _check(rc, what):
    if rc != 0:
        raise EngineError("%s failed (%d): %s" % (what, rc, load_library().ra_last_error().decode()))


def _norm_flag(flag):
    """None or the header's -1: by mode; otherwise on / off (a bare bool(-1) would switch the normalisation ON)"""
    if flag is None or (not isinstance(flag, bool) and isinstance(flag, (int, float)) and flag < 0):
        return -1
    return int(bool(flag))


class Engine:
    """Handle-based engine.  All tensor arguments are torch CUDA tensors on `device`."""

    def __init__(self, nx, last_ring, xrng, yrng, step, nref, mode=RA_MODE_MREF, first_ring=1, ring_skip=1,
                 device=0, chunk=0, interp=RA_INTERP_BILINEAR, normalize_ring=None):
        """interp / normalize_ring: the two hedges of include/ralign.h (ra_options) for the choices of the EMAN2 CPU path that the
        reference tree does not pin -- Util::alrl_ms's interpolation (RA_INTERP_QUADRI: older EMAN2 releases; size-generic kernels)
        and Normalize_ring on / off independent of the mode (None, or the header's -1: by mode)."""
        import torch
        self.torch = torch
        self.lib = load_library()
        self.cfg = RaConfig(int(nx), int(first_ring), int(last_ring), int(ring_skip), float(xrng), float(yrng),
                            float(step), int(nref), int(mode), int(device), int(chunk))
        self.handle = ctypes.c_void_p()
        if interp == RA_INTERP_BILINEAR and _norm_flag(normalize_ring) < 0:
            _check(self.lib.ra_create(ctypes.byref(self.handle), ctypes.byref(self.cfg)), "ra_create")
        else:
            opt = RaOptions(int(interp), _norm_flag(normalize_ring))
            _check(self.lib.ra_create_ex(ctypes.byref(self.handle), ctypes.byref(self.cfg), ctypes.byref(opt)), "ra_create_ex")
        self.nx, self.nref, self.mode, self.device = int(nx), int(nref), int(mode), int(device)
        self.dev = torch.device("cuda", device)

    def close(self):
        if self.handle:
            self.lib.ra_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers
    def _ptr(self, t, dtype=None):
        if t is None:
            return None
        assert t.is_cuda and t.is_contiguous(), "device tensor must be a contiguous CUDA tensor"
        if dtype is not None:
            assert t.dtype == dtype, (t.dtype, dtype)
        return ctypes.c_void_p(t.data_ptr())

    def use_current_stream(self):
        s = self.torch.cuda.current_stream(self.dev)
        _check(self.lib.ra_set_stream(self.handle, ctypes.c_void_p(s.cuda_stream)), "ra_set_stream")

    @property
    def num_shifts(self):
        return self.lib.ra_num_shifts(self.handle)

    @property
    def maxrin(self):
        return self.lib.ra_maxrin(self.handle)

    @property
    def search_path(self):
        """1 = fused particle-resident kernel, 0 = polar + contraction kernel pair, 2 = size-generic kernels"""
        return self.lib.ra_search_path(self.handle)

    @property
    def lcirc(self):
        return self.lib.ra_lcirc(self.handle)

    def new_state(self, n):
        return self.torch.zeros((n, 2), dtype=self.torch.float32, device=self.dev)

    def new_result(self, n):
        return self.torch.zeros((n, 8), dtype=self.torch.int32, device=self.dev)

    @staticmethod
    def result_to_numpy(result):
        return result.cpu().numpy().view(RESULT_DTYPE).reshape(-1)

    # -- API
    def reset_shifts(self, xrng, yrng, step):
        _check(self.lib.ra_reset_shifts(self.handle, xrng, yrng, step), "ra_reset_shifts")

    def set_mask(self, mask):
        """user mask [nx][nx] (CUDA tensor) in place of model_circle(last_ring)"""
        assert mask.shape == (self.nx, self.nx)
        _check(self.lib.ra_set_mask(self.handle, self._ptr(mask, self.torch.float32)), "ra_set_mask")

    def set_normalize_ring(self, flag):
        """Normalize_ring for subsequent searches: True / False, None (or -1) = the mode's default (ra_set_normalize_ring)"""
        _check(self.lib.ra_set_normalize_ring(self.handle, _norm_flag(flag)), "ra_set_normalize_ring")

    @property
    def options(self):
        """(interp, normalize_ring) in force (ra_get_options)"""
        o = RaOptions()
        _check(self.lib.ra_get_options(self.handle, ctypes.byref(o)), "ra_get_options")
        return int(o.interp), int(o.normalize_ring)

    def set_nomirror(self, flag):
        """--nomirror: search the straight orientation only (ormq -> Util.Crosrng_ns)"""
        _check(self.lib.ra_set_nomirror(self.handle, int(bool(flag))), "ra_set_nomirror")

    def set_references(self, refs):
        assert refs.shape == (self.nref, self.nx, self.nx)
        _check(self.lib.ra_set_references(self.handle, self._ptr(refs, self.torch.float32)), "ra_set_references")

    def prepared_references(self):
        out = np.zeros((self.nref, self.lcirc), np.float32)
        _check(self.lib.ra_get_prepared_references(self.handle, out.ctypes.data_as(ctypes.c_void_p)),
               "ra_get_prepared_references")
        return out

    def align(self, particles, state, result, cs=None):
        n = particles.shape[0]
        assert particles.shape[1:] == (self.nx, self.nx) and state.shape == (n, 2) and result.shape == (n, 8)
        csp = None
        if cs is not None:
            csp = (ctypes.c_float * 2)(float(cs[0]), float(cs[1]))
        _check(self.lib.ra_align(self.handle, self._ptr(particles, self.torch.float32), n,
                                 self._ptr(state, self.torch.float32), self._ptr(result, self.torch.int32), csp),
               "ra_align")

    @property
    def search_tiled(self):
        return bool(self.lib.ra_search_tiled(self.handle))

    @property
    def search_l1_tap_rings(self):
        """search_fused_kernel: rings of at most this many samples (64 | 128) read their taps through the vector L1; 0: all from
        LDS (ra_search_l1_tap_rings)"""
        return self.lib.ra_search_l1_tap_rings(self.handle)

    @property
    def search_skips_offsets(self):
        """True when the search evaluates the in-window offsets of a particle only (ra_search_skips_offsets)"""
        return bool(self.lib.ra_search_skips_offsets(self.handle))

    @property
    def search_offsets_per_pass(self):
        """search_path == 3 (rings of 512 samples): 2 = search_duo_kernel, 1 = search_solo_kernel; 0 otherwise"""
        return self.lib.ra_search_offsets_per_pass(self.handle)

    def set_refine(self, threshold):
        """sub-bin angle refinement with the CPU path's arithmetic (ra_set_refine): threshold on |c3| / max |b| of prb1d,
        < 0 = every particle, 0 = off; call before set_references"""
        _check(self.lib.ra_set_refine(self.handle, float(threshold)), "ra_set_refine")

    def state_from_params(self, result, state, cs=None):
        """the reference's state round trip (ra_state_from_params): state <- inverse_transform2 of the float32 parameters
        in `result` (with the centre correction cs folded in first in the reference-free mode)"""
        n = result.shape[0]
        assert state.shape == (n, 2) and result.shape == (n, 8)
        csp = None
        if cs is not None:
            csp = (ctypes.c_float * 2)(float(cs[0]), float(cs[1]))
        _check(self.lib.ra_state_from_params(self.handle, self._ptr(result, self.torch.int32), n, csp,
                                             self._ptr(state, self.torch.float32)), "ra_state_from_params")

    def last_refine_count(self):
        """particles the last search launch re-evaluated in the CPU path's arithmetic (diagnostics; synchronises)"""
        return self.lib.ra_last_refine_count(self.handle)

    def lds_report(self):
        """the LDS ledger (ra_lds_report): one dict per kernel whose dynamic LDS the engine has raised -- kernel, static_bytes (of the
        loaded code object), dynamic_bytes, limit_bytes (per workgroup of the device)"""
        n = self.lib.ra_lds_report(self.handle, None, 0)
        if n < 0:
            _check(n, "ra_lds_report")
        rows = (RaLdsRow * max(n, 1))()
        n = min(n, self.lib.ra_lds_report(self.handle, rows, n))
        return [{"kernel": rows[i].kernel.decode(), "static_bytes": rows[i].static_bytes, "dynamic_bytes": rows[i].dynamic_bytes,
                 "limit_bytes": rows[i].limit_bytes} for i in range(n)]

    def state_from_params_dev(self, result, state, cs_dev):
        """state_from_params with the centre correction in a CUDA tensor [2] (no host value in the path)"""
        n = result.shape[0]
        assert state.shape == (n, 2) and result.shape == (n, 8) and cs_dev.numel() == 2
        _check(self.lib.ra_state_from_params_dev(self.handle, self._ptr(result, self.torch.int32), n,
                                                 self._ptr(cs_dev, self.torch.float32), self._ptr(state, self.torch.float32)),
               "ra_state_from_params_dev")

    def set_class_references(self, refs):
        """class-resident mode: one reference per class, [ncls][nx][nx] (ra_set_class_references)"""
        assert refs.shape[1:] == (self.nx, self.nx)
        _check(self.lib.ra_set_class_references(self.handle, self._ptr(refs, self.torch.float32), int(refs.shape[0])),
               "ra_set_class_references")

    def align_classes(self, particles, state, result, cls):
        """every particle against the reference of its class cls[i] (int32, device), one launch (ra_align_classes)"""
        n = particles.shape[0]
        assert particles.shape[1:] == (self.nx, self.nx) and state.shape == (n, 2) and result.shape == (n, 8) and cls.shape == (n,)
        _check(self.lib.ra_align_classes(self.handle, self._ptr(particles, self.torch.float32), n,
                                         self._ptr(state, self.torch.float32), self._ptr(result, self.torch.int32),
                                         self._ptr(cls, self.torch.int32)), "ra_align_classes")

    def transform_accumulate(self, particles, result, index0=0, aligned=None, sums=None, counts=None):
        n = particles.shape[0]
        _check(self.lib.ra_transform_accumulate(self.handle, self._ptr(particles, self.torch.float32), n, int(index0),
                                                self._ptr(result, self.torch.int32),
                                                self._ptr(aligned, self.torch.float32),
                                                self._ptr(sums, self.torch.float32),
                                                self._ptr(counts, self.torch.int32)), "ra_transform_accumulate")

    def update_references(self, sums, counts, refs, min_count=4):
        _check(self.lib.ra_update_references(self.handle, self._ptr(sums, self.torch.float32),
                                             self._ptr(counts, self.torch.int32), int(min_count),
                                             self._ptr(refs, self.torch.float32)), "ra_update_references")

    def normalize_particles(self, particles):
        _check(self.lib.ra_normalize_particles(self.handle, self._ptr(particles, self.torch.float32),
                                               particles.shape[0]), "ra_normalize_particles")

    def debug_spectra(self, particles, state):
        """ring spectra [n][num_shifts][lcirc] (EMAN2 packing) of the polar / ring-FFT stage alone"""
        n = particles.shape[0]
        out = np.zeros((n, self.num_shifts, self.lcirc), np.float32)
        _check(self.lib.ra_debug_spectra(self.handle, self._ptr(particles, self.torch.float32), n,
                                         self._ptr(state, self.torch.float32), out.ctypes.data_as(ctypes.c_void_p)),
               "ra_debug_spectra")
        return out

    def debug_exact_references(self):
        """(exact reference spectra [nref][lcirc], copy table [nref][2] = (first copy, next copy or -1)) of the sub-bin refinement
        (ra_debug_exact_references)"""
        refx = np.zeros((self.nref, self.lcirc), np.float32)
        dup = np.zeros((self.nref, 2), np.int32)
        _check(self.lib.ra_debug_exact_references(self.handle, refx.ctypes.data_as(ctypes.c_void_p), dup.ctypes.data_as(ctypes.c_void_p)),
               "ra_debug_exact_references")
        return refx, dup

    def debug_finalize(self, cand, nrtile, state, kernel, live, refine_thr, with_list=True):
        """finalize_kernel (kernel 0) or finalize_wave_kernel (1) over hand-built records (ra_debug_finalize): cand CAND_DTYPE, dense
        [n][ent_stride][nrtile] or (live) the in-window offsets' records only; state float32 [n][2].  Returns (results RESULT_DTYPE [n],
        new state [n][2], refine list REFINE_DTYPE [count] in append order -- empty without a list)"""
        cand = np.ascontiguousarray(cand, CAND_DTYPE)
        state = np.ascontiguousarray(state, np.float32)
        n = state.shape[0]
        assert state.shape == (n, 2) and cand.size % int(nrtile) == 0
        res = np.zeros(n, RESULT_DTYPE)
        st = np.zeros((n, 2), np.float32)
        rl = np.zeros(n, REFINE_DTYPE)
        cnt = ctypes.c_int(0)
        _check(self.lib.ra_debug_finalize(self.handle, cand.ctypes.data_as(ctypes.c_void_p), int(nrtile), n,
                                          state.ctypes.data_as(ctypes.c_void_p), int(kernel), int(bool(live)), float(refine_thr),
                                          res.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p),
                                          rl.ctypes.data_as(ctypes.c_void_p) if with_list else None, n, ctypes.byref(cnt)),
               "ra_debug_finalize")
        return res, st, rl[:cnt.value].copy()

    def debug_refine(self, particles, rlist, state, result, cls=None):
        """refine_winner_kernel over the hand-built list rlist (REFINE_DTYPE) against the engine's exact references, in place on the
        CUDA tensors state [n][2] and result [n][8] (ra_debug_refine); cls: int32 CUDA tensor [n], class-resident mode"""
        rlist = np.ascontiguousarray(rlist, REFINE_DTYPE)
        n = particles.shape[0]
        assert particles.shape[1:] == (self.nx, self.nx) and state.shape == (n, 2) and result.shape == (n, 8)
        _check(self.lib.ra_debug_refine(self.handle, self._ptr(particles, self.torch.float32), n, rlist.ctypes.data_as(ctypes.c_void_p),
                                        int(rlist.size), self._ptr(state, self.torch.float32), self._ptr(result, self.torch.int32),
                                        self._ptr(cls, self.torch.int32)), "ra_debug_refine")

    # -- reference update on the device
    def class_fsc(self, sums, counts, min_count=4, masked=False):
        """[freq, fsc, npoints] lists like sp_statistics.fsc / fsc_mask, averaged over the live classes"""
        n = self.lib.ra_fsc_len(self.handle)
        out = np.zeros((3, n), np.float32)
        _check(self.lib.ra_class_fsc(self.handle, self._ptr(sums, self.torch.float32), self._ptr(counts, self.torch.int32),
                                     int(min_count), int(bool(masked)), out.ctypes.data_as(float_ptr)), "ra_class_fsc")
        return [list(map(float, out[0])), list(map(float, out[1])), list(map(float, out[2]))]

    def last_class_fsc(self):
        """per-class curves of the last class_fsc call: (fsc [nref][len], points per shell [nref][len]) (ra_last_class_fsc)"""
        n = self.lib.ra_fsc_len(self.handle)
        out = np.zeros((self.nref, 2, n), np.float32)
        _check(self.lib.ra_last_class_fsc(self.handle, out.ctypes.data_as(float_ptr)), "ra_last_class_fsc")
        return out[:, 0], out[:, 1]

    def class_averages(self, sums, counts, refs, min_count=4):
        _check(self.lib.ra_class_averages(self.handle, self._ptr(sums, self.torch.float32),
                                          self._ptr(counts, self.torch.int32), int(min_count),
                                          self._ptr(refs, self.torch.float32)), "ra_class_averages")

    def class_fsc_fit(self, sums, counts, fit, curve, min_count=4, masked=False, fl_lo=0.12, fl_hi=0.4, aa_hi=0.2):
        """class_fsc + fit_tanh + the clamps of ref_ali2d on the device: fit [5] and curve [3][fsc_len] are CUDA float tensors the
        kernels fill (ra_class_fsc_fit); nothing is read back here"""
        n = self.lib.ra_fsc_len(self.handle)
        assert fit.numel() >= 5 and curve.numel() >= 3 * n
        _check(self.lib.ra_class_fsc_fit(self.handle, self._ptr(sums, self.torch.float32), self._ptr(counts, self.torch.int32),
                                         int(min_count), int(bool(masked)), float(fl_lo), float(fl_hi), float(aa_hi),
                                         self._ptr(fit, self.torch.float32), self._ptr(curve, self.torch.float32)), "ra_class_fsc_fit")

    def filter_references_dev(self, imgs, flaa=None, center=0, cs_in=None, normalize=True, cs_out=None):
        """filter_references with (fl, aa), the centres of center = -1 and the applied centres in CUDA tensors; asynchronous"""
        m = imgs.shape[0]
        _check(self.lib.ra_filter_references_dev(self.handle, self._ptr(imgs, self.torch.float32), m,
                                                 self._ptr(flaa, self.torch.float32), int(center), self._ptr(cs_in, self.torch.float32),
                                                 int(bool(normalize)), self._ptr(cs_out, self.torch.float32)), "ra_filter_references_dev")

    @property
    def fsc_len(self):
        return self.lib.ra_fsc_len(self.handle)

    def filter_references(self, imgs, fl, aa, center=0, cs_in=None, normalize=True):
        """in place on imgs [m][nx][nx]; returns the applied centres [m][2]"""
        m = imgs.shape[0]
        cin = None
        if cs_in is not None:
            cin = np.ascontiguousarray(cs_in, np.float32).reshape(m, 2)
        cout = np.zeros((m, 2), np.float32)
        _check(self.lib.ra_filter_references(self.handle, self._ptr(imgs, self.torch.float32), m, float(fl), float(aa),
                                             int(center), cin.ctypes.data_as(float_ptr) if cin is not None else None,
                                             int(bool(normalize)), cout.ctypes.data_as(float_ptr)), "ra_filter_references")
        return cout

    def sync(self):
        _check(self.lib.ra_sync(self.handle), "ra_sync")

    def kernel_time(self, enable=True):
        """returns (ms_ccf, launches_ccf, ms_polar, launches_polar) since the last call and
        (re)arms HIP-event timing of the two hot kernels on the engine's stream."""
        a = ctypes.c_double(); b = ctypes.c_double(); na = ctypes.c_int(); nb = ctypes.c_int()
        _check(self.lib.ra_kernel_time(self.handle, int(enable), ctypes.byref(a), ctypes.byref(na), ctypes.byref(b),
                                       ctypes.byref(nb)), "ra_kernel_time")
        return a.value, na.value, b.value, nb.value
