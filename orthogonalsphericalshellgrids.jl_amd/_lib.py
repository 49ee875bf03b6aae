"""ctypes binding of the shared libraries of the package: the product, libtripolar_hip.so (include/tripolar_hip.h), and the operator libraries.

This is the ONLY compute backend of the package: if a shared library is missing or a call
fails, the caller gets an exception -- there is no CPU or PyTorch fallback by design.

The convention, stated once: the operator library <name> is libtripolar_hip_<name>.so beside this file, built from csrc/tpg_<name>.hip through
csrc/<name>.map (csrc/Makefile lists the names), it exports what include/tripolar_hip_<name>.h declares, and its error channel is
tpg_<name>_last_error.  Here it is one table <NAME>_SIGNATURES of every symbol that header declares, (restype, argtypes) each, and one line
<name>_lib, check_<name> = _library("<name>", <NAME>_SIGNATURES), which makes its loader and its status checker, sets <NAME>_LIB_PATH and
enters a record in LIBRARIES, the registry of every library in the order of definition: what build() loads and tests/test_library_table.py
checks against the headers, the maps and the built files.
"""
import collections
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


# the product: every symbol include/tripolar_hip.h declares, (restype, argtypes)
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

# the operator libraries, <NAME>_SIGNATURES each: every symbol include/tripolar_hip_<name>.h declares
OPERATORS_SIGNATURES = {
    "tpg_operators_last_error": (C.c_char_p, []),
    "tpg_vertical_vorticity": (_i, [_vp] * 7 + [C.c_double] + _geom + [_i, _vp]),
}

CONTINUITY_SIGNATURES = {
    "tpg_continuity_last_error": (C.c_char_p, []),
    "tpg_w_from_continuity": (_i, [_vp] * 9 + [C.c_double] + _geom + [_i, _vp]),
}

BAROTROPIC_SIGNATURES = {
    "tpg_barotropic_last_error": (C.c_char_p, []),
    "tpg_barotropic_mode": (_i, [_vp] * 5 + _geom + [_i, _i, _vp]),
    "tpg_barotropic_correction": (_i, [_vp] * 9 + [C.c_double] + _geom + [_i, _i, _vp]),
}

FREE_SURFACE_SIGNATURES = {
    "tpg_free_surface_last_error": (C.c_char_p, []),
    "tpg_free_surface_substep": (_i, [_vp] * 19 + [C.c_double] * 3 + [_i] * 6 + [_vp]),
}

TPG_AB2_EULER, TPG_AB2_STORE_PREVIOUS = 1, 2                 # flag bits of both calls
TIMESTEP_SIGNATURES = {
    "tpg_timestep_last_error": (C.c_char_p, []),
    "tpg_ab2_step_velocities": (_i, [_vp] * 11 + [C.c_double] * 2 + [_i] + _geom + [_i, _i, _vp]),
    "tpg_ab2_step_fields": (_i, [C.POINTER(_vp)] * 3 + [_i] + [C.c_double] * 2 + [_i] + _geom + [_i, _vp]),
}

TPG_ADVECTION_CENTERED2 = 0                                  # `scheme` of tpg_tracer_advection_tendency: the only one built
ADVECTION_SIGNATURES = {
    "tpg_advection_last_error": (C.c_char_p, []),
    "tpg_tracer_advection_tendency": (_i, [C.POINTER(_vp)] * 2 + [_i] + [_vp] * 8 + [C.c_double, _i] + _geom + [_i, _vp]),
}

TPG_MOMENTUM_ENSTROPHY_CONSERVING = 0                        # `scheme` of tpg_momentum_advection_tendency: the only one built
MOMENTUM_SIGNATURES = {
    "tpg_momentum_last_error": (C.c_char_p, []),
    "tpg_momentum_advection_tendency": (_i, [_vp] * 16 + [C.c_double, _i] + _geom + [_i, _vp]),
}

WENO_SIGNATURES = {
    "tpg_weno_last_error": (C.c_char_p, []),
    "tpg_weno_tracer_advection_tendency": (_i, [C.POINTER(_vp)] * 2 + [_i] + [_vp] * 8 + [C.c_double] + _geom + [_i, _vp]),
}

WENO_MOMENTUM_SIGNATURES = {
    "tpg_weno_momentum_last_error": (C.c_char_p, []),
    "tpg_weno_momentum_advection_tendency": (_i, [_vp] * 16 + [C.c_double] + _geom + [_i, _vp]),
}

WENO_XYZ_SIGNATURES = {
    "tpg_weno_xyz_last_error": (C.c_char_p, []),
    "tpg_weno_xyz_tracer_advection_tendency": (_i, [C.POINTER(_vp)] * 2 + [_i] + [_vp] * 8 + [C.c_double] + _geom + [_i, _vp]),
}

WENO_VI_SIGNATURES = {
    "tpg_weno_vi_last_error": (C.c_char_p, []),
    "tpg_weno_vi_momentum_advection_tendency": (_i, [_vp] * 16 + [C.c_double] + _geom + [_i, _vp]),
}

WENO_VS_SIGNATURES = {
    "tpg_weno_vs_last_error": (C.c_char_p, []),
    "tpg_weno_vs_momentum_advection_tendency": (_i, [_vp] * 16 + [C.c_double] + _geom + [_i, _vp]),
}

TPG_CORIOLIS_ENSTROPHY_CONSERVING, TPG_CORIOLIS_ENERGY_CONSERVING = 0, 1     # `coriolis_scheme` of tpg_hydrostatic_tendencies
TPG_TENDENCY_ADD, TPG_TENDENCY_WRITE = 0, 1                                  # its `mode`
HYDROSTATIC_SIGNATURES = {
    "tpg_hydrostatic_last_error": (C.c_char_p, []),
    "tpg_hydrostatic_tendencies": (_i, [_vp] * 14 + [C.c_double, _i, _i] + _geom + [_i, _vp]),
}

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


# one record of LIBRARIES: the file names under include/ and csrc/, the NAME of the module-level variable that holds the path, the table, the two functions
Library = collections.namedtuple("Library", "header map path_global signatures load check")
LIBRARIES = {}


def _library(name, signatures, handle=None, path=None, last_error=None, header=None, map=None):
    """(loader, checker) of the library `name`, entered in LIBRARIES.  Everything else follows from the name (see the module docstring); only the
    product spells it out.  `handle` and `path` NAME module-level variables, read at every call: the cached handle (None: not loaded yet;
    tools.testlib swaps _lib) and the path, which a caller may assign before the first load.  `last_error`: its error channel."""
    handle, path, last_error = handle or f"_{name}", path or f"{name.upper()}_LIB_PATH", last_error or f"tpg_{name}_last_error"
    g = globals()
    g.setdefault(handle, None)
    g.setdefault(path, os.path.join(_HERE, f"libtripolar_hip_{name}.so"))

    def load():
        if g[handle] is None:
            g[handle] = _load(g[path], signatures)
        return g[handle]

    def check(status):
        if status != 0:
            raise TripolarHipError(status, getattr(load(), last_error)().decode("utf-8", "replace"))

    load.__doc__ = f"Load the library at {path} (once); ImportError if it has not been built."
    LIBRARIES[name] = Library(header or f"tripolar_hip_{name}.h", map or f"{name}.map", path, signatures, load, check)
    return load, check


lib, check = _library("product", SIGNATURES, handle="_lib", path="LIB_PATH", last_error="tpg_last_error", header="tripolar_hip.h", map="exports.map")
operators_lib, check_operators = _library("operators", OPERATORS_SIGNATURES)
continuity_lib, check_continuity = _library("continuity", CONTINUITY_SIGNATURES)
barotropic_lib, check_barotropic = _library("barotropic", BAROTROPIC_SIGNATURES)
free_surface_lib, check_free_surface = _library("free_surface", FREE_SURFACE_SIGNATURES)
timestep_lib, check_timestep = _library("timestep", TIMESTEP_SIGNATURES)
advection_lib, check_advection = _library("advection", ADVECTION_SIGNATURES)
momentum_lib, check_momentum = _library("momentum", MOMENTUM_SIGNATURES)
weno_lib, check_weno = _library("weno", WENO_SIGNATURES)
weno_momentum_lib, check_weno_momentum = _library("weno_momentum", WENO_MOMENTUM_SIGNATURES)
weno_xyz_lib, check_weno_xyz = _library("weno_xyz", WENO_XYZ_SIGNATURES)
weno_vi_lib, check_weno_vi = _library("weno_vi", WENO_VI_SIGNATURES)
weno_vs_lib, check_weno_vs = _library("weno_vs", WENO_VS_SIGNATURES)
hydrostatic_lib, check_hydrostatic = _library("hydrostatic", HYDROSTATIC_SIGNATURES)
vertical_diffusion_lib, check_vertical_diffusion = _library("vertical_diffusion", VERTICAL_DIFFUSION_SIGNATURES)


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
