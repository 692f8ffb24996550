"""ctypes binding of libdiffsep_hip.so (include/diffsep_hip.h).  No fallback: if the HIP library
is missing or a call fails, this raises — the product path never routes around the GPU code."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# Two builds of the same sources: the 16-bit storage format of dtype code 1 is bfloat16 in libdiffsep_hip.so and IEEE half
# precision in libdiffsep_hip_f16.so (csrc/Makefile, -DDS_HALF_F16).  DIFFSEP_LIB overrides the first one (profiling builds).
LIB_PATH = os.environ.get("DIFFSEP_LIB", os.path.join(os.path.dirname(_HERE), "libdiffsep_hip.so"))
LIB_PATHS = {"bf16": LIB_PATH, "f16": os.environ.get("DIFFSEP_LIB_F16", os.path.join(os.path.dirname(_HERE), "libdiffsep_hip_f16.so"))}

F32, BF16 = 0, 1
F32_SPLIT = 2  # fp32 tensors; matrix products as 3 bf16 MFMAs on hi / lo halves (include/diffsep_hip.h)
F16 = 3        # Python-side only: dtype code 1 (16-bit storage) of the half-precision build
F64 = 4        # float64 rows: an output type of diffsep_resample only
SDE_MIX, SDE_PRIORMIX = 0, 1
PRED_REVERSE_DIFFUSION, PRED_EULER_MARUYAMA, PRED_NONE = 0, 1, 2
CORR_ALD2, CORR_NONE, CORR_ALD, CORR_LANGEVIN = 0, 1, 2, 3
PREDICTORS = {"reverse_diffusion": PRED_REVERSE_DIFFUSION, "euler_maruyama": PRED_EULER_MARUYAMA, "none": PRED_NONE}
CORRECTORS = {"ald2": CORR_ALD2, "none": CORR_NONE, "ald": CORR_ALD, "langevin": CORR_LANGEVIN}


class ModelConfig(C.Structure):
    _fields_ = [("nf", C.c_int32), ("num_sources", C.c_int32), ("n_levels", C.c_int32), ("ch_mult", C.c_int32 * 8),
                ("num_res_blocks", C.c_int32), ("attn_resolution", C.c_int32), ("n_fft", C.c_int32),
                ("hop", C.c_int32), ("spec_abs_exponent", C.c_float), ("spec_factor", C.c_float),
                ("dtype", C.c_int32)]


class SdeConfig(C.Structure):
    _fields_ = [("kind", C.c_int32), ("ndim", C.c_int32), ("d_lambda", C.c_float), ("sigma_min", C.c_float),
                ("sigma_max", C.c_float), ("avg_len", C.c_int32)]


class SamplerConfig(C.Structure):
    _fields_ = [("N", C.c_int32), ("corrector_steps", C.c_int32), ("snr", C.c_float), ("eps", C.c_float),
                ("denoise", C.c_int32), ("predictor", C.c_int32), ("corrector", C.c_int32)]


class SamplerExt(C.Structure):
    _fields_ = [("lengths_host", C.POINTER(C.c_int64)), ("seeds_host", C.POINTER(C.c_uint64)),
                ("tail_engine", C.c_void_p), ("tail_steps", C.c_int32), ("head_steps", C.c_int32)]


ODE_RK45, ODE_RK23 = 0, 1
ODE_METHODS = {"RK45": ODE_RK45, "RK23": ODE_RK23}
ODE_WORKSPACE_BYTES = 16384
# diffsep_ode_sample_fixed: the fixed-step methods and the network evaluations of an M-step solve
ODEF_EULER, ODEF_HEUN, ODEF_MIDPOINT, ODEF_RK4, ODEF_AB2 = 0, 1, 2, 3, 4
ODEF_METHODS = {"euler": ODEF_EULER, "heun": ODEF_HEUN, "midpoint": ODEF_MIDPOINT, "rk4": ODEF_RK4, "ab2": ODEF_AB2}
ODEF_ERR_METHODS = ("heun", "midpoint", "ab2")  # those with an embedded Euler step (err_out)


def odef_nfe(method, steps):
    """network evaluations of a fixed-step solve (the denoise evaluation is not counted)"""
    return {"euler": steps, "heun": 2 * steps, "midpoint": 2 * steps, "rk4": 4 * steps, "ab2": steps + 1}[method]


# diffsep_ode_sample_expint: the exponential integrators of the same solve (steps network evaluations each) and the width of a
# row of their coefficient table
EXPINT_DDIM, EXPINT_DPMPP2M = 0, 1
EXPINT_METHODS = {"ddim": EXPINT_DDIM, "dpmpp2m": EXPINT_DPMPP2M}
EXPINT_ERR_METHODS = ("dpmpp2m",)  # err_out: the step minus its DDIM step
EXPINT_COEFS = 12


class OdeConfig(C.Structure):  # diffsep_ode_config
    _fields_ = [("rtol", C.c_double), ("atol", C.c_double), ("eps", C.c_double), ("first_step", C.c_double),
                ("max_step", C.c_double), ("method", C.c_int32), ("max_nfe", C.c_int32), ("denoise", C.c_int32),
                ("N", C.c_int32)]


class OdeExt(C.Structure):  # diffsep_ode_ext
    _fields_ = [("lengths_host", C.POINTER(C.c_int64)), ("seeds_host", C.POINTER(C.c_uint64))]


class OdeInfo(C.Structure):  # diffsep_ode_info
    _fields_ = [("nfev", C.c_int32), ("n_accepted", C.c_int32), ("n_rejected", C.c_int32), ("status", C.c_int32),
                ("t_final", C.c_double)]


# route codes of diffsep_gn_apply (DIFFSEP_GN_* of include/diffsep_hip.h): the dispatch's choice, or one kernel of csrc/norm.hip
GN_ROUTES = {"auto": 0, "apply": 1, "block2x2": 2, "down_strip4": 3, "down_strip8": 4, "down_tiled4": 5, "down_tiled8": 6,
             "up_tiled": 7}

PIT_NONE, PIT_TRUE_MIX, PIT_MEAN0 = 0, 1, 2
WARM_SCALE_NONE, WARM_SCALE_LS = 0, 1       # diffsep_warm_start: the gain fit
WARM_MEAN_MIX, WARM_MEAN_ESTIMATE = 0, 1    # ... and where the perturbation's source average comes from
WARM_SCALES = {"none": WARM_SCALE_NONE, "ls": WARM_SCALE_LS}
WARM_MEANS = {"mix": WARM_MEAN_MIX, "estimate": WARM_MEAN_ESTIMATE}


class LossConfig(C.Structure):  # diffsep_loss_config
    _fields_ = [("pit_mode", C.c_int32), ("redefine_z", C.c_int32)]


class ProfRecord(C.Structure):  # diffsep_prof_record
    _fields_ = [("kernel", C.c_char * 128), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
                ("Cout", C.c_int32), ("taps", C.c_int32), ("skip_cin", C.c_int32), ("has_res", C.c_int32),
                ("cls", C.c_int32), ("_pad", C.c_int32), ("flops", C.c_double), ("bytes", C.c_double), ("ms", C.c_double)]


TRACE_FIELDS, TRACE_NAME_BYTES = 9, 160  # diffsep_engine_debug_trace: int64 fields and name bytes per record


class DiffsepError(RuntimeError):
    pass


# ---- marshalling shared by engine.py and ops.py: what a C argument is made of, each once
def _stream_ptr(device=None):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def sde_config(d):
    """dict(kind, ndim, d_lambda, sigma_min, sigma_max[, avg_len]) -> SdeConfig"""
    return SdeConfig(d.get("kind", SDE_MIX), d["ndim"], d["d_lambda"], d["sigma_min"], d["sigma_max"], d.get("avg_len", 0))


def host_array(values, dtype, n, what):
    """(contiguous numpy array [n] of dtype, its typed pointer) for a `*_host` argument; the caller keeps the array alive"""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(values, dtype=dtype))
    assert a.shape == (n,), f"{what} must be [B]"
    return a, a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def ode_info_dict(info):
    return dict(nfev=info.nfev, n_accepted=info.n_accepted, n_rejected=info.n_rejected, status=info.status, t_final=info.t_final)


_lib = None

_P, _I, _L, _F, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint64
_SIGS = {
    "diffsep_last_error": (C.c_char_p, []),
    "diffsep_version": (C.c_char_p, []),
    "diffsep_param_count": (_I, [C.POINTER(ModelConfig)]),
    "diffsep_param_info": (_I, [C.POINTER(ModelConfig), _I, C.c_char_p, _I, C.POINTER(_L), C.POINTER(_I),
                                C.POINTER(_L)]),
    "diffsep_param_total": (_L, [C.POINTER(ModelConfig)]),
    "diffsep_engine_create": (_I, [C.POINTER(ModelConfig), _P, _L, C.POINTER(_P)]),
    "diffsep_engine_destroy": (None, [_P]),
    "diffsep_engine_device_bytes": (_L, [_P]),
    "diffsep_engine_reserve": (_I, [_P, _I, _L, _P]),
    "diffsep_engine_debug_absmax": (_I, [_P, C.POINTER(C.c_double), _I, C.POINTER(_I)]),
    "diffsep_engine_debug_arena": (_I, [_P, C.POINTER(_P), C.POINTER(_L), C.POINTER(_L)]),
    "diffsep_engine_debug_trace": (_I, [_P, C.POINTER(_L), C.c_char_p, _I, C.POINTER(_I)]),
    "diffsep_num_frames": (_I, [C.POINTER(ModelConfig), _L]),
    "diffsep_padded_frames": (_I, [C.POINTER(ModelConfig), _L]),
    "diffsep_score_forward": (_I, [_P, _P, _P, _P, _P, _I, _L, _P]),
    "diffsep_backbone_forward": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "diffsep_pc_sample": (_I, [_P, C.POINTER(SdeConfig), C.POINTER(SamplerConfig), _P, _P, _I, _L, _P, _U64, _P,
                               C.POINTER(_I), _P]),
    "diffsep_pc_sample_ex": (_I, [_P, C.POINTER(SdeConfig), C.POINTER(SamplerConfig), C.POINTER(SamplerExt), _P, _P, _I,
                                  _L, _P, _U64, _P, C.POINTER(_I), _P]),
    "diffsep_pc_sample_trace": (_I, [_P, C.POINTER(SdeConfig), C.POINTER(SamplerConfig), C.POINTER(SamplerExt), _P, _P, _I,
                                     _L, _P, _U64, _P, C.POINTER(_I), _I, C.POINTER(_I), _P, _P, _P, _P, _P]),
    "diffsep_pc_sample_from": (_I, [_P, C.POINTER(SdeConfig), C.POINTER(SamplerConfig), C.POINTER(SamplerExt), _P, _P, _I,
                                    _L, _P, _U64, _P, C.POINTER(_I), _I, C.POINTER(_I), _P, _P, _P, _P, _P, _I, _I, _P]),
    "diffsep_ode_sample": (_I, [_P, C.POINTER(SdeConfig), C.POINTER(OdeConfig), _P, _P, _P, _U64, _P, _I, _L,
                                C.POINTER(OdeInfo), _P]),
    "diffsep_ode_sample_each": (_I, [_P, C.POINTER(SdeConfig), C.POINTER(OdeConfig), C.POINTER(OdeExt), _P, _P, _P, _U64, _P,
                                     _I, _L, C.POINTER(OdeInfo), C.POINTER(_I), _P]),
    "diffsep_ode_sample_fixed": (_I, [_P, C.POINTER(SdeConfig), _I, _I, C.c_double, C.c_double, _I, _I, C.POINTER(SamplerExt), _P,
                                      _P, _P, _U64, C.POINTER(C.c_double), _P, _P, _I, _L, C.POINTER(_I), _P]),
    "diffsep_ode_sample_expint": (_I, [_P, C.POINTER(SdeConfig), _I, _I, C.c_double, C.c_double, _I, _I, C.POINTER(SamplerExt), _P,
                                       _P, _P, _U64, C.POINTER(C.c_double), _P, _P, _I, _L, C.POINTER(_I), _P]),
    "diffsep_expint_coefficients": (_I, [C.POINTER(SdeConfig), _I, _I, C.c_double, C.c_double, C.POINTER(C.c_double), _P]),
    "diffsep_expint_update_each": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _L, _P, _L,
                                        _P]),
    "diffsep_ode_tableau": (_I, [_I, _P, _P, _P, _P, C.POINTER(_I), C.POINTER(_I)]),
    "diffsep_ode_stage_update": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_double, _P, _P, _I,
                                      _I, _L, _P]),
    "diffsep_ode_error_norm": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.c_double,
                                    C.c_double, C.c_double, _P, _I, _I, _L, _P, _L, _P]),
    "diffsep_ode_stage_update_each": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P,
                                           _I, _I, _L, _P]),
    "diffsep_ode_error_norm_each": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P,
                                         C.c_double, C.c_double, _P, _I, _I, _L, _P, _L, _P]),
    "diffsep_engine_set_graph": (_I, [_P, _I]),
    "diffsep_set_option": (_I, [C.c_char_p, _L]),
    "diffsep_engine_set_option": (_I, [_P, C.c_char_p, _L]),
    "diffsep_engine_get_option": (_L, [_P, C.c_char_p]),
    "diffsep_engine_profile_begin": (_I, [_P]),
    "diffsep_engine_profile_end": (_I, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_L),
                                        C.POINTER(C.c_double)]),
    "diffsep_engine_profile_end_n": (_I, [_P, _I, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_L),
                                          C.POINTER(C.c_double), C.POINTER(_I)]),
    "diffsep_num_kernel_classes": (_I, []),
    "diffsep_engine_profile_records": (_I, [_P, C.POINTER(ProfRecord), _I, C.POINTER(_I)]),
    "diffsep_time_embedding": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _L, _P]),
    "diffsep_dense_projection": (_I, [_P, _P, _P, C.POINTER(_I), _I, _P, _I, _I, _I, _P, _L, _P]),
    "diffsep_upfirdn2d": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "diffsep_groupnorm_act": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _I, _I, _I, _P, _L, _P]),
    "diffsep_conv2d": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _I, _P]),
    "diffsep_groupnorm_stats": (_I, [_P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _I, _P, _L, _P]),
    "diffsep_conv2d_fused": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F,
                                  _I, _P, _I, _P, _P, _P, _P, _I, _P]),
    "diffsep_conv2d_chunk": (_I, [_I, _I]),
    "diffsep_gemm_nt": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _I, _P]),
    "diffsep_last_conv_kernel": (C.c_char_p, []),
    "diffsep_gn_finalize_acc": (_I, [_P, _I, _P, _I, _I, _L, _I, _F, _P, _P, _P, _P, _P]),
    "diffsep_gn_apply": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "diffsep_gn_route_name": (C.c_char_p, [_I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I]),
    "diffsep_conv3x3_streamed": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P, _P,
                                      _P, _P, _P, _P, _P, _I, _P]),
    "diffsep_conv3x3_regweight": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P,
                                       _P]),
    "diffsep_attn_fused": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "diffsep_frag_index": (_L, [_I, _I, _I, _I, _I]),
    "diffsep_frag_index_split": (_L, [_I, _I, _I, _I, _I, _I]),
    "diffsep_resblock_forward": (_I, [_I, _I, _I, _I, _I, _I, _P, _L, _P, _P, _P, _I, _I, _I, _P]),
    "diffsep_attnblock_forward": (_I, [_I, _I, _P, _L, _P, _P, _I, _I, _I, _P]),
    "diffsep_attention": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _L, _P]),
    "diffsep_stft_pack": (_I, [_P, _P, _P, _I, _I, _L, _I, _I, _F, _F, _I, _I, _I, _I, _P, _L, _P]),
    "diffsep_istft_unpack": (_I, [_P, _P, _I, _I, _L, _I, _I, _F, _F, _I, _I, _I, _P, _L, _P]),
    "diffsep_stft_pack_ex": (_I, [_P, _P, _P, _I, _I, _L, _I, _I, _F, _F, _I, _I, _I, _I, _P, _L, _P, _I]),
    "diffsep_istft_unpack_ex": (_I, [_P, _P, _I, _I, _L, _I, _I, _F, _F, _I, _I, _I, _P, _L, _P, _I, _P, _P, _P, _I]),
    "diffsep_sde_sigma_mix": (_I, [_P, _P, _I, _L, _I, _P]),
    "diffsep_sde_prior": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _I, _I, _L, _P, _P]),
    "diffsep_sde_corrector_update": (_I, [C.POINTER(SdeConfig), _F, _P, _P, _P, _P, _P, _P, _I, _I, _L, _P, _I, _P]),
    "diffsep_sde_predictor_update": (_I, [C.POINTER(SdeConfig), _I, _P, _P, _P, _P, _P, _P, _I, _I, _L, _P, _I, _P]),
    "diffsep_sde_coefficients": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _P, _P, _I, _I, _L, _F, _F, _P]),
    "diffsep_sde_mean": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _I, _I, _L, _P]),
    "diffsep_sde_std": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _I, _I, _L, _P]),
    "diffsep_sde_mult_std": (_I, [_P, _P, _P, _I, _I, _L, _I, _P]),
    "diffsep_sde_mult_std_inv": (_I, [_P, _P, _P, _I, _I, _L, _I, _P]),
    "diffsep_sde_perturb": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _P, _P, _P, _I, _P, _U64, _U64, _P, _P, _I, _I, _L, _P]),
    "diffsep_score_loss_workspace_bytes": (_L, [_I, _I, _L]),
    "diffsep_score_loss_reduce": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _I, _L, _P,
                                       _L, _P]),
    "diffsep_score_loss": (_I, [_P, C.POINTER(SdeConfig), C.POINTER(LossConfig), _P, _P, _P, _P, _P, _U64, _P, _P, _P, _P, _P,
                                _P, _I, _L, _P, _L, _P]),
    "diffsep_score_loss_validate": (_I, [C.POINTER(ModelConfig), C.POINTER(LossConfig), _I, _L, _P, _L]),
    "diffsep_sde_reverse_drift": (_I, [_P, _P, _P, _P, _I, _L, _I, _I, _P]),
    "diffsep_sde_langevin_update": (_I, [_F, _P, _P, _P, _P, _P, _I, _L, _P, _L, _P]),
    "diffsep_normalize_batch": (_I, [_P, _P, _P, _P, _I, _L, _P]),
    "diffsep_scale_output": (_I, [_P, _P, _I, _I, _L, _P]),
    "diffsep_gram": (_I, [_P, _P, _P, _I, _I, _L, _P]),
    "diffsep_stoi_workspace_bytes": (_L, [_I, _I, _L, _I]),
    "diffsep_stoi": (_I, [_P, _P, _P, _I, _I, _L, _P, _P, _I, _I, _P, _L, _P]),
    "diffsep_composite_workspace_bytes": (_L, [_I, _I, _L, _I]),
    "diffsep_composite": (_I, [_P, _P, _P, _P, _L, _I, _I, _L, _P, _P, _I, _P, _L, _P]),
    "diffsep_bss_eval_workspace_bytes": (_L, [_I, _I, _L, _I]),
    "diffsep_bss_eval": (_I, [_P, _P, _P, _P, _P, _I, _I, _L, _P, _P, _I, C.c_double, _P, _L, _P]),
    "diffsep_resample_ratio": (_I, [_I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "diffsep_resample_length": (_L, [_L, _I, _I]),
    "diffsep_resample_design": (_I, [_I, _I, _P, _I]),
    "diffsep_resampler_create": (_I, [_I, _I, _P, _I, C.POINTER(_P)]),
    "diffsep_resampler_destroy": (None, [_P]),
    "diffsep_resample": (_I, [_P, _P, _L, _P, _L, _I, _L, _P, _I, _P, _I, _P]),
    "diffsep_longform_plan": (_I, [_L, _L, _L, C.POINTER(_L), _I]),
    "diffsep_longform_locate": (_I, [_L, _L, _L, _L, C.POINTER(_I), C.POINTER(_L), C.POINTER(_L)]),
    "diffsep_longform_workspace_bytes": (_L, [_I, _I]),
    "diffsep_longform_stitch": (_I, [_P, _I, _I, _L, _L, _L, _P, _P, _P, _P, _L, _P]),
    "diffsep_ensemble_workspace_bytes": (_L, [_I, _I, _I]),
    "diffsep_ensemble": (_I, [_P, _P, _P, _I, _I, _I, _L, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    "diffsep_warm_start_workspace_bytes": (_L, [_I, _I]),
    "diffsep_warm_start": (_I, [C.POINTER(SdeConfig), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U64, _I, _I, _P, _P, _P, _I, _I,
                                _L, _P, _L, _P]),
    "diffsep_randn": (_I, [_P, _L, _U64, _U64, _P]),
    "diffsep_randn_batch": (_I, [_P, _I, _I, _L, _P, _P, _U64, _P]),
    "diffsep_convert": (_I, [_P, _P, _L, _I, _I, _P]),
}
EXPORTS = tuple(_SIGS.keys())


def lib(kind="bf16"):
    """Load (once) and return the HIP library of a storage variant ("bf16": libdiffsep_hip.so, "f16":
    libdiffsep_hip_f16.so); raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = {}
    if kind not in _lib:
        path = LIB_PATHS[kind]
        if not os.path.exists(path):
            raise DiffsepError(f"{path} not found: build it with __graft_entry__.build() or "
                               "`make -C diffusion-separation_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
        # On a GPU box torch must have brought the HIP runtime up BEFORE this library is loaded: loaded first (e.g.
        # __graft_entry__.build() followed by smoke() in one process), its device calls then failed with "no
        # ROCm-capable device is detected" (measured; the library and torch share one libamdhip64).  No-op without a GPU.
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:
            pass
        l = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib[kind] = l
    return _lib[kind]


def check(rc, l=None):
    if rc != 0:
        raise DiffsepError((l or lib()).diffsep_last_error().decode("utf-8", "replace"))


def call(L, name, *args):
    """L.<name>(*args), then check() against L itself: the error text always comes from the library that was called"""
    check(getattr(L, name)(*args), L)


def half_kind(dtype_code):
    """storage variant of a dtype code: F16 lives in the half-precision build, everything else in the default one"""
    return "f16" if dtype_code == F16 else "bf16"


def model_config(nf=64, num_sources=2, ch_mult=(1, 1, 2, 2, 2, 2, 2), num_res_blocks=2, attn_resolution=16,
                 n_fft=510, hop=128, spec_abs_exponent=0.5, spec_factor=0.33, dtype=F32):
    c = ModelConfig()
    c.nf, c.num_sources, c.n_levels = nf, num_sources, len(ch_mult)
    for i, m in enumerate(ch_mult):
        c.ch_mult[i] = m
    c.num_res_blocks, c.attn_resolution, c.n_fft, c.hop = num_res_blocks, attn_resolution, n_fft, hop
    c.spec_abs_exponent, c.spec_factor, c.dtype = spec_abs_exponent, spec_factor, dtype
    return c


def ode_tableau(method="RK45"):
    """(A [ns,ns], B [ns], C [ns], E [ns+1], n_stages, error_estimator_order) of diffsep_ode_tableau: the Butcher tableau
    the device solver uses, as scipy's rk.py holds it.  Host code only (no GPU needed)."""
    import numpy as np
    l = lib()
    code = ODE_METHODS[method]
    ns, eo = C.c_int32(), C.c_int32()
    call(l, "diffsep_ode_tableau", code, None, None, None, None, C.byref(ns), C.byref(eo))
    n = ns.value
    A, B, Cc, E = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n + 1)
    call(l, "diffsep_ode_tableau", code, *(a.ctypes.data_as(C.c_void_p) for a in (A, B, Cc, E)), None, None)
    return A, B, Cc, E, n, eo.value


def expint_coefficients(sde, method, steps, t_start=None, eps=3e-2, timesteps=None):
    """diffsep_expint_coefficients: the float64 table [steps, EXPINT_COEFS] of "ddim" / "dpmpp2m" on the grid the fixed-step
    solve builds from (steps, t_start, eps) or takes from timesteps (steps + 1 times); row i = cx_A cd_A w0_A w1_A | cx_P
    cd_P w0_P w1_P | alpha_A ev_A alpha_P ev_P at t_i.  sde: the dict of sde_config.  Host code only (no GPU needed)."""
    import numpy as np
    M = int(steps)
    ts = None
    if timesteps is not None:
        ts = np.ascontiguousarray(timesteps, dtype=np.float64).reshape(-1)
        if ts.size != M + 1:
            raise DiffsepError(f"expint_coefficients: timesteps must hold steps + 1 = {M + 1} times, got {ts.size}")
    out = np.zeros((max(M, 0), EXPINT_COEFS))
    call(lib(), "diffsep_expint_coefficients", C.byref(sde_config(sde)), EXPINT_METHODS.get(method, method), M,
         float(t_start) if t_start is not None else 0.0, float(eps),
         ts.ctypes.data_as(C.POINTER(C.c_double)) if ts is not None else None, out.ctypes.data_as(C.c_void_p))
    return out
