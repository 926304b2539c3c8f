"""`ais_estimate` with the reference's surface (l2hmc/utils/ais.py:30-82, annealed importance sampling after Wu et al.
2016), on the one-launch kernel behind `DynamicsSampler.ais`."""
from .dynamics import Dynamics
from .dynamics_sampler import DynamicsSampler


def ais_estimate(init_energy, final_energy, anneal_steps, initial_x, step_size=0.5, leapfrogs=25, refresh=False,
                 refreshment=0.1, seed=42):
    """utils/ais.py:30-42 -> (log_ratio, mean_alpha) as :79 returns them: the estimate of log(Z_final / Z_init) from
    `anneal_steps` steps of the schedule linspace(0, 1, anneal_steps + 1)[1:], and the mean accept probability.
    The two energies are the library's distribution objects: `init_energy` a `Gaussian` the rows of `initial_x`
    [B, x_dim] were drawn from, `final_energy` anything with `get_energy_function()` the one-launch kernels hold
    (GMM, Gaussian, RoughWell, GaussianFunnel, x_dim <= 8).  The transitions are those of
    `Dynamics(x_dim, energy, eps=step_size, hmc=True, trajectory_length=leapfrogs)` (:58, whose stale `T=` keyword is
    the trajectory length); `refresh` / `refreshment` as :52-55; `seed` is the dynamics' Philox seed.  Not served, as
    in `DynamicsSampler.ais`: `aux`, `num_splits`; `x_dim` is the width of `initial_x`."""
    x_dim = int(initial_x.shape[1])
    dyn = Dynamics(x_dim, final_energy.get_energy_function(), trajectory_length=leapfrogs, eps=step_size, hmc=True,
                   seed=seed)
    out = DynamicsSampler(dyn).ais(anneal_steps, init_energy, initial_x,
                                   refresh=float(refreshment) if refresh else None)
    return out["log_ratio"], out["mean_accept"]
