"""ctypes binding of libtripolar_hip.so (include/tripolar_hip.h), of the five operator libraries beside it
(include/tripolar_hip_operators.h, _continuity.h, _barotropic.h, _free_surface.h, _timestep.h) and of the tendency libraries (_advection.h,
_momentum.h, _weno.h, _weno_momentum.h, _weno_xyz.h, _weno_vi.h, _weno_vs.h, _hydrostatic.h, _vertical_diffusion.h).

This is the ONLY compute backend of the package: if a shared library is missing or a call
fails, the caller gets an exception -- there is no CPU or PyTorch fallback by design.

A library is described once -- its path, its signature table, its *_last_error symbol -- and _library() makes its loader and its
status checker from that: lib / check, operators_lib / check_operators, and so on for continuity, barotropic, free_surface, timestep,
advection, momentum, weno, weno_momentum, weno_xyz, weno_vi, weno_vs, hydrostatic and vertical_diffusion.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtripolar_hip.so")

TPG_F32, TPG_F64 = 0, 1
TPG_CENTER, TPG_FACE = 0, 1
TPG_MAX_FIELDS = 16
TPG_SIDE_SOUTH, TPG_SIDE_BOTTOM, TPG_SIDE_TOP = 1, 2, 4      # tpg_fill_bounded_halos side bits
TPG_BC_VALUE, TPG_BC_GRADIENT = 1, 2                         # tpg_fill_value_gradient_halos kinds
TPG_BUILD_TABLES_VALID = 1        # tpg_params.reserved flag

# enum tpg_array (order of src/tripolar_grid.jl:308-328 in the reference)
ARRAY_NAMES = (
    "lambda_cc", "lambda_fc", "lambda_cf", "lambda_ff",
    "phi_cc", "phi_fc", "phi_cf", "phi_ff",
    "dx_cc", "dx_fc", "dx_cf", "dx_ff",
    "dy_cc", "dy_cf", "dy_fc", "dy_ff",
    "az_cc", "az_fc", "az_cf", "az_ff",
)

STATUS = {
    0: "TPG_OK", -1: "TPG_ERR_INVALID_ARGUMENT", -2: "TPG_ERR_ODD_NLAMBDA", -3: "TPG_ERR_BAD_PARTITION",
    -4: "TPG_ERR_WORKSPACE", -5: "TPG_ERR_UNSUPPORTED", -6: "TPG_ERR_NOT_NORTH", -7: "TPG_ERR_RCCL",
}
TPG_COMM_ID_BYTES = 128


class TpgParams(C.Structure):
    """struct tpg_params"""
    _fields_ = [
        ("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32),
        ("Hx", C.c_int32), ("Hy", C.c_int32), ("Hz", C.c_int32),
        ("southernmost_latitude", C.c_double),
        ("north_poles_latitude", C.c_double),
        ("first_pole_longitude", C.c_double),
        ("radius", C.c_double),
        ("ft", C.c_int32), ("jstart", C.c_int32), ("jend", C.c_int32), ("reserved", C.c_int32),
    ]


class TripolarHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"libtripolar_hip: {STATUS.get(status, status)}: {message}")
        self.status = status


# every symbol include/tripolar_hip.h declares: (restype, argtypes)
_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
_geom = [_i] * 6
SIGNATURES = {
    "tpg_version": (_i, []),
    "tpg_last_error": (C.c_char_p, []),
    "tpg_status_string": (C.c_char_p, [_i]),
    "tpg_build_grid_workspace_bytes": (_sz, [C.POINTER(TpgParams)]),
    "tpg_build_grid": (_i, [C.POINTER(TpgParams), C.POINTER(_vp), _vp, _sz, _vp]),
    "tpg_zipper_fill": (_i, [C.POINTER(_vp), _i, C.POINTER(C.c_int8), C.POINTER(C.c_int8), C.POINTER(C.c_int32)]
                        + _geom + [_i, _i, _i, _vp]),
    "tpg_zipper_fill_timed": (_i, [C.POINTER(_vp), _i, C.POINTER(C.c_int8), C.POINTER(C.c_int8), C.POINTER(C.c_int32)]
                              + _geom + [_i, _i, _i, _vp, _vp, _vp]),
    "tpg_event_create": (_i, [C.POINTER(_vp)]),
    "tpg_event_destroy": (_i, [_vp]),
    "tpg_event_elapsed_ms": (_i, [_vp, _vp, C.POINTER(C.c_float)]),
    "tpg_periodic_x_fill": (_i, [C.POINTER(_vp), _i] + _geom + [_i, _vp]),
    "tpg_fill_halo_regions": (_i, [C.POINTER(_vp), _i, C.POINTER(C.c_int8), C.POINTER(C.c_int8), C.POINTER(C.c_int32)]
                              + _geom + [_i, _i, _vp]),
    "tpg_fill_halo_regions_timed": (_i, [C.POINTER(_vp), _i, C.POINTER(C.c_int8), C.POINTER(C.c_int8), C.POINTER(C.c_int32)]
                                    + _geom + [_i, _i, _vp, _vp, _vp]),
    "tpg_fill_bounded_halos": (_i, [C.POINTER(_vp), _i, C.POINTER(C.c_uint8)] + _geom + [_i, _vp]),
    "tpg_fill_value_gradient_halos": (_i, [C.POINTER(_vp), _i, _i, C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(_vp), _vp,
                                           C.c_double, C.c_double] + _geom + [_i, _vp]),
    "tpg_fill_open_faces": (_i, [C.POINTER(_vp), _i, C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(_vp)] + _geom + [_i, _vp]),
    "tpg_immersed_column_counts": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "tpg_mask_immersed_fields": (_i, [C.POINTER(_vp), _i, C.POINTER(_vp), C.POINTER(C.c_int8), C.POINTER(C.c_double)] + _geom + [_i, _vp]),
    "tpg_reduce_workspace_bytes": (_sz, [_i] * 4),
    "tpg_field_extrema": (_i, [C.POINTER(_vp), _i, C.POINTER(_vp), C.POINTER(C.c_int8), _vp, _vp, _sz] + _geom + [_i, _vp]),
    "tpg_cell_advection_timescale": (_i, [_vp] * 9 + [_sz] + _geom + [_i, _vp]),
    "tpg_y_halo_buffer_elems": (_sz, [_i] * 6),
    "tpg_pack_y_halo": (_i, [C.POINTER(_vp), _i, _vp, _i] + _geom + [_i, _vp]),
    "tpg_unpack_y_halo": (_i, [C.POINTER(_vp), _i, _vp, _i] + _geom + [_i, _vp]),
    "tpg_comm_available": (_i, []),
    "tpg_comm_unique_id": (_i, [_vp]),
    "tpg_comm_init_rank": (_i, [C.POINTER(_vp), _i, _vp, _i]),
    "tpg_comm_destroy": (_i, [_vp]),
    "tpg_halo_exchange_y": (_i, [_vp, _i, _i, C.POINTER(_vp), _i, _vp, _vp, _vp, _vp] + _geom + [_i, _vp]),
    "tpg_halo_exchange_y_peers": (_i, [_vp, _i, _i, C.POINTER(_vp), _i, _vp, _vp, _vp, _vp] + _geom + [_i, _vp]),
    "tpg_halo_exchange_y_pipelined": (_i, [_vp, _i, _i, C.POINTER(_vp), _i, _vp, _vp, _vp, _vp] + _geom + [_i, _vp, _vp, _i]),
    "tpg_halo_exchange_y_pipelined_peers": (_i, [_vp, _i, _i, C.POINTER(_vp), _i, _vp, _vp, _vp, _vp] + _geom + [_i, _vp, _vp, _i]),
    "tpg_fill_halo_regions_distributed_pipelined": (_i, [_vp, _i, _i, C.POINTER(_vp), _i, C.POINTER(C.c_int8), C.POINTER(C.c_int8),
                                                         C.POINTER(C.c_int32), _vp, _vp, _vp, _vp] + _geom + [_i, _vp, _vp, _i]),
    "tpg_fill_halo_regions_distributed_pipelined_peers": (_i, [_vp, _i, _i, _i, C.POINTER(_vp), _i, C.POINTER(C.c_int8), C.POINTER(C.c_int8),
                                                               C.POINTER(C.c_int32), _vp, _vp, _vp, _vp] + _geom + [_i, _vp, _vp, _i]),
    "tpg_fill_halo_regions_distributed": (_i, [_vp, _i, _i, C.POINTER(_vp), _i, C.POINTER(C.c_int8), C.POINTER(C.c_int8), C.POINTER(C.c_int32),
                                               _vp, _vp, _vp, _vp] + _geom + [_i, _vp]),
    "tpg_fill_halo_regions_distributed_peers": (_i, [_vp, _i, _i, _i, C.POINTER(_vp), _i, C.POINTER(C.c_int8), C.POINTER(C.c_int8),
                                                     C.POINTER(C.c_int32), _vp, _vp, _vp, _vp] + _geom + [_i, _vp]),
    "tpg_nonorthogonality_angle": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "tpg_convert_frame": (_i, [_vp] * 8 + [_i] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_operators.h declares (libtripolar_hip_operators.so: a library of its own beside the product's)
OPERATORS_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_operators.so")
OPERATOR_SIGNATURES = {
    "tpg_operators_last_error": (C.c_char_p, []),
    "tpg_vertical_vorticity": (_i, [_vp] * 7 + [C.c_double] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_continuity.h declares (libtripolar_hip_continuity.so: the third library, no test build)
CONTINUITY_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_continuity.so")
CONTINUITY_SIGNATURES = {
    "tpg_continuity_last_error": (C.c_char_p, []),
    "tpg_w_from_continuity": (_i, [_vp] * 9 + [C.c_double] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_barotropic.h declares (libtripolar_hip_barotropic.so: the fourth library, no test build)
BAROTROPIC_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_barotropic.so")
BAROTROPIC_SIGNATURES = {
    "tpg_barotropic_last_error": (C.c_char_p, []),
    "tpg_barotropic_mode": (_i, [_vp] * 5 + _geom + [_i, _i, _vp]),
    "tpg_barotropic_correction": (_i, [_vp] * 9 + [C.c_double] + _geom + [_i, _i, _vp]),
}

# every symbol include/tripolar_hip_free_surface.h declares (libtripolar_hip_free_surface.so: the fifth library, no test build)
FREE_SURFACE_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_free_surface.so")
FREE_SURFACE_SIGNATURES = {
    "tpg_free_surface_last_error": (C.c_char_p, []),
    "tpg_free_surface_substep": (_i, [_vp] * 19 + [C.c_double] * 3 + [_i] * 6 + [_vp]),
}

# every symbol include/tripolar_hip_timestep.h declares (libtripolar_hip_timestep.so: the sixth library, no test build)
TIMESTEP_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_timestep.so")
TPG_AB2_EULER, TPG_AB2_STORE_PREVIOUS = 1, 2                 # flag bits of both calls
TIMESTEP_SIGNATURES = {
    "tpg_timestep_last_error": (C.c_char_p, []),
    "tpg_ab2_step_velocities": (_i, [_vp] * 11 + [C.c_double] * 2 + [_i] + _geom + [_i, _i, _vp]),
    "tpg_ab2_step_fields": (_i, [C.POINTER(_vp)] * 3 + [_i] + [C.c_double] * 2 + [_i] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_advection.h declares (libtripolar_hip_advection.so: the seventh library, no test build)
ADVECTION_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_advection.so")
TPG_ADVECTION_CENTERED2 = 0                                  # `scheme` of tpg_tracer_advection_tendency: the only one built
ADVECTION_SIGNATURES = {
    "tpg_advection_last_error": (C.c_char_p, []),
    "tpg_tracer_advection_tendency": (_i, [C.POINTER(_vp)] * 2 + [_i] + [_vp] * 8 + [C.c_double, _i] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_momentum.h declares (libtripolar_hip_momentum.so: the eighth library, no test build)
MOMENTUM_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_momentum.so")
TPG_MOMENTUM_ENSTROPHY_CONSERVING = 0                        # `scheme` of tpg_momentum_advection_tendency: the only one built
MOMENTUM_SIGNATURES = {
    "tpg_momentum_last_error": (C.c_char_p, []),
    "tpg_momentum_advection_tendency": (_i, [_vp] * 16 + [C.c_double, _i] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_weno.h declares (libtripolar_hip_weno.so: the ninth library, no test build)
WENO_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_weno.so")
WENO_SIGNATURES = {
    "tpg_weno_last_error": (C.c_char_p, []),
    "tpg_weno_tracer_advection_tendency": (_i, [C.POINTER(_vp)] * 2 + [_i] + [_vp] * 8 + [C.c_double] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_weno_momentum.h declares (libtripolar_hip_weno_momentum.so: the tenth library, no test build)
WENO_MOMENTUM_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_weno_momentum.so")
WENO_MOMENTUM_SIGNATURES = {
    "tpg_weno_momentum_last_error": (C.c_char_p, []),
    "tpg_weno_momentum_advection_tendency": (_i, [_vp] * 16 + [C.c_double] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_weno_xyz.h declares (libtripolar_hip_weno_xyz.so: the eleventh library, no test build)
WENO_XYZ_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_weno_xyz.so")
WENO_XYZ_SIGNATURES = {
    "tpg_weno_xyz_last_error": (C.c_char_p, []),
    "tpg_weno_xyz_tracer_advection_tendency": (_i, [C.POINTER(_vp)] * 2 + [_i] + [_vp] * 8 + [C.c_double] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_weno_vi.h declares (libtripolar_hip_weno_vi.so: the twelfth library, no test build)
WENO_VI_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_weno_vi.so")
WENO_VI_SIGNATURES = {
    "tpg_weno_vi_last_error": (C.c_char_p, []),
    "tpg_weno_vi_momentum_advection_tendency": (_i, [_vp] * 16 + [C.c_double] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_weno_vs.h declares (libtripolar_hip_weno_vs.so: the thirteenth library, no test build)
WENO_VS_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_weno_vs.so")
WENO_VS_SIGNATURES = {
    "tpg_weno_vs_last_error": (C.c_char_p, []),
    "tpg_weno_vs_momentum_advection_tendency": (_i, [_vp] * 16 + [C.c_double] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_hydrostatic.h declares (libtripolar_hip_hydrostatic.so: the fourteenth library, no test build)
HYDROSTATIC_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_hydrostatic.so")
TPG_CORIOLIS_ENSTROPHY_CONSERVING, TPG_CORIOLIS_ENERGY_CONSERVING = 0, 1     # `coriolis_scheme` of tpg_hydrostatic_tendencies
TPG_TENDENCY_ADD, TPG_TENDENCY_WRITE = 0, 1                                  # its `mode`
HYDROSTATIC_SIGNATURES = {
    "tpg_hydrostatic_last_error": (C.c_char_p, []),
    "tpg_hydrostatic_tendencies": (_i, [_vp] * 14 + [C.c_double, _i, _i] + _geom + [_i, _vp]),
}

# every symbol include/tripolar_hip_vertical_diffusion.h declares (libtripolar_hip_vertical_diffusion.so: the fifteenth library, no test build)
VERTICAL_DIFFUSION_LIB_PATH = os.path.join(_HERE, "libtripolar_hip_vertical_diffusion.so")
TPG_KAPPA_CONSTANT, TPG_KAPPA_PROFILE, TPG_KAPPA_FIELD = 0, 1, 2             # `kappa_form` of tpg_vertical_implicit_diffusion
TPG_VDIFF_AUTO, TPG_VDIFF_ON_CHIP, TPG_VDIFF_STREAMED = 0, 1, 2              # its `path`
VERTICAL_DIFFUSION_SIGNATURES = {
    "tpg_vertical_diffusion_last_error": (C.c_char_p, []),
    "tpg_vertical_diffusion_on_chip_levels": (_i, [_i, _i]),
    "tpg_vertical_implicit_diffusion": (_i, [C.POINTER(_vp), _i, _vp, C.c_double, _i, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _i] + _geom + [_i, _vp]),
}


def bind(path, signatures):
    """dlopen `path` and declare `signatures` on it (AttributeError if the ABI is incomplete)"""
    handle = C.CDLL(path)
    for name, (restype, argtypes) in signatures.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = restype, argtypes
    return handle


def _load(path, signatures):
    """bind `path`; raise loudly if it has not been built (python __graft_entry__.py): no library of the package has a torch fallback"""
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: the HIP extension is the only backend of this package. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C orthogonalsphericalshellgrids.jl_amd/csrc`).")
    return bind(path, signatures)


def _library(handle, path, signatures, last_error):
    """(loader, checker) of one library.  `handle` and `path` NAME module-level variables, read at every call: the cached handle (None: not
    loaded yet; tools.testlib swaps _lib) and the path, which a caller may assign before the first load.  `last_error`: its error channel."""
    g = globals()
    g.setdefault(handle, None)

    def load():
        if g[handle] is None:
            g[handle] = _load(g[path], signatures)
        return g[handle]

    def check(status):
        if status != 0:
            raise TripolarHipError(status, getattr(load(), last_error)().decode("utf-8", "replace"))

    load.__doc__ = f"Load the library at {path} (once); ImportError if it has not been built."
    return load, check


lib, check = _library("_lib", "LIB_PATH", SIGNATURES, "tpg_last_error")
operators_lib, check_operators = _library("_operators", "OPERATORS_LIB_PATH", OPERATOR_SIGNATURES, "tpg_operators_last_error")
continuity_lib, check_continuity = _library("_continuity", "CONTINUITY_LIB_PATH", CONTINUITY_SIGNATURES, "tpg_continuity_last_error")
barotropic_lib, check_barotropic = _library("_barotropic", "BAROTROPIC_LIB_PATH", BAROTROPIC_SIGNATURES, "tpg_barotropic_last_error")
free_surface_lib, check_free_surface = _library("_free_surface", "FREE_SURFACE_LIB_PATH", FREE_SURFACE_SIGNATURES, "tpg_free_surface_last_error")
timestep_lib, check_timestep = _library("_timestep", "TIMESTEP_LIB_PATH", TIMESTEP_SIGNATURES, "tpg_timestep_last_error")
advection_lib, check_advection = _library("_advection", "ADVECTION_LIB_PATH", ADVECTION_SIGNATURES, "tpg_advection_last_error")
OPERATOR_LIBRARIES = (operators_lib, continuity_lib, barotropic_lib, free_surface_lib, timestep_lib)
momentum_lib, check_momentum = _library("_momentum", "MOMENTUM_LIB_PATH", MOMENTUM_SIGNATURES, "tpg_momentum_last_error")
weno_lib, check_weno = _library("_weno", "WENO_LIB_PATH", WENO_SIGNATURES, "tpg_weno_last_error")
TENDENCY_LIBRARIES = (advection_lib, momentum_lib, weno_lib)             # what produces the tendencies the AB2 step consumes
weno_momentum_lib, check_weno_momentum = _library("_weno_momentum", "WENO_MOMENTUM_LIB_PATH", WENO_MOMENTUM_SIGNATURES,
                                                  "tpg_weno_momentum_last_error")
MOMENTUM_TENDENCY_LIBRARIES = (momentum_lib, weno_momentum_lib)          # the two vorticity schemes of the velocity tendencies
weno_xyz_lib, check_weno_xyz = _library("_weno_xyz", "WENO_XYZ_LIB_PATH", WENO_XYZ_SIGNATURES, "tpg_weno_xyz_last_error")
WENO_TRACER_LIBRARIES = (weno_lib, weno_xyz_lib)                         # the two WENO schemes of the tracer tendency: centred in z, WENO in z
# upwinding in every term of the velocity tendency.  Not in MOMENTUM_TENDENCY_LIBRARIES: its call takes dz_c where those two take dz_f
weno_vi_lib, check_weno_vi = _library("_weno_vi", "WENO_VI_LIB_PATH", WENO_VI_SIGNATURES, "tpg_weno_vi_last_error")
# the same call with VelocityStencil smoothness of the vorticity reconstruction: the drivers' WENOVectorInvariant(vorticity_order = 5)
weno_vs_lib, check_weno_vs = _library("_weno_vs", "WENO_VS_LIB_PATH", WENO_VS_SIGNATURES, "tpg_weno_vs_last_error")
# the Coriolis and hydrostatic pressure-gradient tendencies, accumulated into what an advection call left in Gu, Gv
hydrostatic_lib, check_hydrostatic = _library("_hydrostatic", "HYDROSTATIC_LIB_PATH", HYDROSTATIC_SIGNATURES, "tpg_hydrostatic_last_error")
# the vertically implicit diffusion step: the column solve after the AB2 update of u, v and the tracers
vertical_diffusion_lib, check_vertical_diffusion = _library("_vertical_diffusion", "VERTICAL_DIFFUSION_LIB_PATH", VERTICAL_DIFFUSION_SIGNATURES,
                                                            "tpg_vertical_diffusion_last_error")


def ft_of(dtype):
    import torch
    if dtype == torch.float64:
        return TPG_F64
    if dtype == torch.float32:
        return TPG_F32
    raise TypeError(f"unsupported element type {dtype}: Float32 or Float64 only")


def current_stream_ptr(device):
    """hipStream_t of torch's current stream on `device` (so torch.cuda.Event sees our kernels)."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr_table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
