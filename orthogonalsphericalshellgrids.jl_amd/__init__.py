"""orthogonalsphericalshellgrids.jl_amd -- MI355X-native TripolarGrid metric precompute and Zipper
halo fill behind the surface of CliMA/OrthogonalSphericalShellGrids.jl.

The reference exports exactly `TripolarGrid` and `ZipperBoundaryCondition`
(src/OrthogonalSphericalShellGrids.jl:4); the other names are the Oceananigans-side pieces a caller
needs around them (Field constructors, fill_halo_regions!, locations, architectures).
All numerics run in hand-written HIP kernels (csrc/, C ABI in include/tripolar_hip.h).
"""
from .boundary_conditions import (BoundaryCondition, Center, Face, FieldBoundaryConditions, Zipper,
                                  ZipperBoundaryCondition, PeriodicBoundaryCondition, bc_str,
                                  Flux, FluxBoundaryCondition, NoFluxBoundaryCondition,
                                  Value, ValueBoundaryCondition, Gradient, GradientBoundaryCondition,
                                  Open, OpenBoundaryCondition, ImpenetrableBoundaryCondition, is_open,
                                  apply_y_north_bc, regularize_field_boundary_conditions, sign,
                                  validate_boundary_condition_location, is_flux, is_gradient, is_value,
                                  is_zipper)
from .grids import (CPU, GPU, convert_to_0_360, Distributed, Partition, OrthogonalSphericalShellGrid, R_Earth, Tripolar,
                    TripolarGrid, is_tripolar, local_row_range, local_sizes, reconstruct_global_grid, share_tables,
                    with_halo, x_domain, y_domain, RightConnected, FullyConnected, Bounded,
                    PeriodicTopology, GridFittedBottom, ImmersedBoundaryGrid)
from .fields import (CenterField, Field, HaloFillPlan, XFaceField, YFaceField, ZFaceField, fill_halo_regions,
                     halo_fill_plan, interior, set_, immersed_mask_plan, mask_immersed_field)
from .distributed import (LoopbackMailbox, PendingExchange, RcclComm, check_band_widths, exchange_plan, exchange_y_halos,
                          torch_distributed_transport)
from .geometry import convert_to_latlong_frame, convert_to_native_frame, nonorthogonality_angle
from .reductions import (AdvectionTimescalePlan, ExtremaPlan, TimeStepWizard, advection_timescale_plan, cell_advection_timescale,
                         extrema_plan, field_extrema, grid_summary, maximum, minimum, minimum_xspacing, minimum_yspacing, summary,
                         z_all_face_spacings, z_face_spacings)
from .operators import VerticalVorticityField, VorticityPlan, compute_, vertical_vorticity, vorticity_plan
from .continuity import (ContinuityPlan, HorizontalDivergenceField, compute_w_from_continuity, continuity_plan, horizontal_divergence,
                         z_center_spacings)
from .barotropic import (BarotropicCorrectionPlan, BarotropicModePlan, barotropic_correction, barotropic_correction_plan,
                         barotropic_mode_plan, column_depth_table, compute_barotropic_mode)
from .free_surface import (SplitExplicitFreeSurface, SplitExplicitSubcyclePlan, split_explicit_subcycle_plan, split_explicit_substep)
from .time_stepping import (Ab2StepPlan, Ab2VelocityStepPlan, ab2_step_fields, ab2_step_plan, ab2_step_velocities, ab2_velocity_step_plan)
from .advection import TracerAdvectionPlan, tracer_advection_plan, tracer_advection_tendency
from .momentum import MomentumAdvectionPlan, momentum_advection_plan, momentum_advection_tendency
from .weno import (WENO, Centered, FluxFormAdvection, WenoTracerAdvectionPlan, weno_tracer_advection_plan,
                   weno_tracer_advection_tendency)
from .weno_momentum import (DefaultStencil, EnergyConserving, EnstrophyConserving, VectorInvariant, VelocityStencil, WenoMomentumAdvectionPlan,
                            WENOVectorInvariant, weno_momentum_advection_plan, weno_momentum_advection_tendency)
from .weno_xyz import WenoXyzTracerAdvectionPlan, weno_xyz_tracer_advection_plan, weno_xyz_tracer_advection_tendency
from .weno_vi import (OnlySelfUpwinding, WenoViMomentumAdvectionPlan, weno_vi_momentum_advection_plan,
                      weno_vi_momentum_advection_tendency)
from .weno_vs import WenoVsMomentumAdvectionPlan, weno_vs_momentum_advection_plan, weno_vs_momentum_advection_tendency
from .hydrostatic import (BuoyancyTracer, HydrostaticPressurePlan, HydrostaticSphericalCoriolis, HydrostaticTendenciesPlan,
                          coriolis_parameter, hydrostatic_tendencies, hydrostatic_tendencies_plan, update_hydrostatic_pressure)
from .vertical_diffusion import (ExplicitTimeDiscretization, ImplicitStepPlan, VerticalImplicitDiffusionPlan, VerticalScalarDiffusivity,
                                 VerticallyImplicitTimeDiscretization, implicit_step_plan, vertical_implicit_diffusion,
                                 vertical_implicit_diffusion_plan)
from .diffusion import DiffusiveTendencyPlan, HorizontalScalarDiffusivity, diffusive_tendency, diffusive_tendency_plan
from .mixing import (ConvectiveAdjustmentVerticalDiffusivity, ExponentialRiDependentTapering, HyperbolicTangentRiDependentTapering,
                     MixedImplicitStepPlan, PiecewiseLinearRiDependentTapering, RiBasedVerticalDiffusivity, VerticalMixingPlan,
                     mixed_implicit_step_plan, vertical_mixing_diffusivities, vertical_mixing_plan)

__all__ =["TripolarGrid", "ZipperBoundaryCondition"]
