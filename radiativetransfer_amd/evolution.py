"""Time-dependent ionisation: the reference's loop with its equilibrium update replaced by an advance over dt.

A step is what an iteration of the reference's loop is (equiSources.f90:1811-1819) -- zero the rates, trace the point sources, make
the opacities from the medium, sweep the diffuse field into J -- followed by StellarTransfer.advance_rate_equations_device in
place of solveRateEquations.  Everything stays on the device; per step only the two masses of hydrogen_mass() come back.

With thermal=..., the temperature is advanced over the same dt after the species (StellarTransfer.advance_temperature_device),
operator-split: the species of the thermal step are the new ones, its J and point rates the step's.  With
thermal=dict(..., coupled=dict(eta=..., max_subcycles=...)) the two are one call, StellarTransfer.advance_thermochemistry_device:
each leaf is subcycled on the device as finely as its own time scales ask.

With recombination=dict(share=...), every step makes the source function of the ground-state recombination photons from the gas
state as it stands (StellarTransfer.recombination_source_device) between the opacities and the sweep, which carries it: case-A
coefficients with the photons they emit, in place of the on-the-spot approximation of case B.

The coupling is explicit: the rates, J and S of a step are those of the state at its start, held fixed over dt.  The chemistry
itself is implicit and stable for any dt; the ionisation front is not resolved in time unless dt is short against the time the
front takes to cross a cell."""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import numpy as np


def evolve(st, dt: float, nsteps: int, sources: Optional[Tuple[Sequence[int], Sequence[float]]] = None, directions=None, beta=None, uvb=None,
           ksi=None, substeps: int = 1, on_step: Optional[Callable] = None, thermal: Optional[dict] = None, recombination: Optional[dict] = None):
    """Advance the medium of the StellarTransfer `st` over nsteps steps of dt seconds each.

    st          a StellarTransfer with grid, medium (with rho), rate coefficients, temperature and, for sources, rate tables set
    sources     (cells, ndot): 0-based cell-array indices of the stars and their photon rates, or None
    directions  (phi, theta, weight) of the diffuse sweep
    beta        [3][nnu] cross sections per species and frequency group (compute_opacities_from_medium); nnu must be 3
    uvb         [nnu] the background's intensity entering the box
    ksi         [3][3] = [group][ksi24, ksi25, ksi26]
    substeps    implicit steps per dt, at the rates of the step's start
    thermal     None: the temperature stays what set_temperature gave, and the sequence of library calls is as without it.
                dict(gamma=[3][3], tmin=, tmax=, hydro_heating=bool): each step ends, after the ionisation advance, with
                advance_temperature_device over the same dt and substeps, with the same J and point rates (gamma[group][gammaHI,
                gammaHeI, gammaHeII] of uvb_beta_table; needs set_cooling_coefficients, and thermal_equilibrium for hydro_heating);
                the next step's chemistry reads the new temperature.  With coupled=dict(eta=, max_subcycles=) in it, ONE call,
                advance_thermochemistry_device, takes the place of the two: species and temperature of a leaf advance together over
                subcycles of the leaf's own (`substeps` is then not used); without `coupled` the calls are exactly the two above
    recombination  None: no emission, and the sequence of library calls is as without it.  dict(share=[3][3]): each step calls
                recombination_source_device(ksi, share) after compute_opacities_from_medium and before the sweep
                (share[ion][group]; needs set_ground_recombination, and rate coefficients of case A for the ions that emit).
                Emission is switched off again (set_source_function(None), a host-side switch) once the step's sweep has
                carried it, so every step's pass writes the emission field itself, and on return and on an exception: a later sweep
                of the caller's carries no stale S
    on_step     called as on_step(step, st, J) after each step, J the step's [3][ncell] device tensor (for inspection; the rates of
                the step are still on the device)

    Returns (times, neutral): times[nsteps + 1] in seconds from 0 and neutralHydrogenMass / totalHydrogenMass at each."""
    import torch

    if directions is None or beta is None or uvb is None or ksi is None:
        raise ValueError("evolve needs directions, beta, uvb and ksi")
    if nsteps < 0:
        raise ValueError("nsteps must not be negative")
    phi, theta, weight = directions
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    if beta.ndim != 2 or beta.shape != (3, 3):
        raise ValueError("beta must have shape [3][3]: the update takes J in three frequency groups")
    coupled = None if thermal is None else thermal.get("coupled")
    J = torch.empty((3, st.ncell), dtype=torch.float64, device="cuda")  # (the current device, which is the context's by default)
    stream = torch.cuda.current_stream()

    def fraction():
        neutral, total = st.hydrogen_mass()
        return neutral / total

    times, neutral = [0.0], [fraction()]
    try:
        for step in range(nsteps):
            st.set_zero_rates()
            if sources is not None:
                st.point_sources(*sources)
            st.compute_opacities_from_medium(beta)
            if recombination is not None:
                st.recombination_source_device(ksi, recombination["share"])
            st.transport_device(phi, theta, weight, uvb, J.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            if recombination is not None:
                st.set_source_function(None)      # the sweep has carried the step's S: the next step's pass writes the field itself again
            if coupled is not None:
                st.advance_thermochemistry_device(dt, J.data_ptr(), ksi, thermal["gamma"], use_point_rates=True, eta=coupled.get("eta", 0.1),
                                                  max_subcycles=coupled.get("max_subcycles", 64), tmin=thermal.get("tmin", 1.0),
                                                  tmax=thermal.get("tmax", 1.0e9), hydro_heating=bool(thermal.get("hydro_heating", False)))
            else:
                st.advance_rate_equations_device(dt, J.data_ptr(), ksi, use_point_rates=True, substeps=substeps)
            if thermal is not None and coupled is None:
                st.advance_temperature_device(dt, J.data_ptr(), thermal["gamma"], use_point_rates=True, substeps=substeps,
                                              tmin=thermal.get("tmin", 1.0), tmax=thermal.get("tmax", 1.0e9),
                                              hydro_heating=bool(thermal.get("hydro_heating", False)))
            if on_step is not None:
                on_step(step, st, J)
            times.append((step + 1) * float(dt))
            neutral.append(fraction())
    finally:
        if recombination is not None:
            st.set_source_function(None)      # emission was the steps' alone: a later sweep of the caller's carries no stale S
    return np.array(times), np.array(neutral)
