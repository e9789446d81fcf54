"""The run every posterior sampler shares: the prologue up to the flat start sample, the step loop
with its noise source, the epilogue.  A sampler's ``__call__`` hands ``run_sampler`` its step
factory and what is its own; the noise sources (``rng`` / ``seed`` / ``noise_fn``) are described in
``samplers.dps``."""

from __future__ import annotations

from typing import Callable

import torch
from torch import Tensor

from samplers_amd import _hip
from samplers_amd.networks.base import host_timesteps
from samplers_amd.samplers.utils.batch_view import BatchView

NoiseFn = Callable[[str, int, tuple], Tensor]


def draw_seed() -> int:
    """A 63-bit seed from torch's default CPU generator (reproducible under manual_seed)."""
    return int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())


def initial_sample(shape: tuple, device: torch.device, *, rng: str, seed: int, sample_offset: int,
                   noise_fn: NoiseFn | None) -> Tensor:
    """x_T ~ N(0, I) (``dps.py:83-87``)."""
    if noise_fn is not None:
        return noise_fn("init", -1, shape).to(device=device, dtype=torch.float32).contiguous()
    if rng == "torch":
        return torch.randn(size=shape, device=device, dtype=torch.float32)
    if rng != "philox":
        raise ValueError(f"rng must be 'philox' or 'torch', got {rng!r}")
    lib = _hip.load_library()
    x = torch.empty(shape, device=device, dtype=torch.float32)
    n = x[0].numel() if shape[0] else 0
    if shape[0]:
        _hip.check(lib.sp_randn(_hip.ptr(x), shape[0], n, seed, -1, sample_offset,
                                _hip.stream_of(x)), "sp_randn")
    return x


def step_noise(x: Tensor, i: int, *, rng: str, noise_fn: NoiseFn | None) -> Tensor | None:
    """ξ of step ``i``: injected, torch's draw, or None (the step's kernel draws by Philox)."""
    if noise_fn is not None:
        return noise_fn("step", i, tuple(x.shape)).to(device=x.device, dtype=torch.float32)
    return torch.randn_like(x) if rng == "torch" else None


def run_steps(step, x: Tensor, ts, tail: tuple, *, rng: str, seed: int, noise_fn: NoiseFn | None,
              sample_offset: int, callback: Callable[[int, Tensor], None] | None = None) -> None:
    """``i = len(ts)−1 … 2``: ``step(x, i, ts[i], ts[i−1], *tail, …)`` in place; ``callback(i, x)``
    after each."""
    for i in range(len(ts) - 1, 1, -1):
        step(x, i, ts[i], ts[i - 1], *tail, xi=step_noise(x, i, rng=rng, noise_fn=noise_fn),
             seed=seed, sample_offset=sample_offset)
        if callback is not None:
            callback(i, x)


def run_sampler(sampler, inverse_problem, make_step, *, num_sampling_steps: int,
                num_reconstructions: int, condition, rng: str, seed: int | None,
                noise_fn: NoiseFn | None, sample_offset: int, keep_reconstruction_dim: bool = False,
                require: str | None = None, anchored: bool = False, data_shape=None,
                y_shape=None, advance=None, finish=None) -> Tensor:
    """One posterior-sampling run of ``sampler`` (a ``PosteriorSampler``).

    ``make_step(net, y_rows)`` builds the step object from the fp32 observation rows
    ``(batch, *y_shape)`` (``y_shape``: the operator's unless given).  ``require`` names the sampler
    where the observation must be a device tensor before the step is built.  ``anchored`` steps
    take ``ts[0]`` as their fifth positional argument.  ``data_shape`` is the shape of one working
    sample (the operator's ``x_shape`` unless given).  ``advance(step, x, ts, seed, loop)`` replaces
    the plain ``loop()`` over the steps; ``finish(x0)`` replaces the epilogue (unflatten, squeeze the
    reconstruction axis when 1, the network's dtype) of the flat ``predict_x0`` result."""
    operator = inverse_problem.operator
    batch_shape = inverse_problem.batch_shape
    view = BatchView(batch_shape=batch_shape, num_samples=num_reconstructions,
                     data_shape=operator.x_shape if data_shape is None else data_shape)
    net = sampler._network
    net.set_sampling_parameters(num_sampling_steps=num_sampling_steps,
                                num_reconstructions=num_reconstructions,
                                batch_size=view.batch_size)
    net.set_condition(condition=condition)
    try:
        obs = inverse_problem.observation
        if require is not None:
            _hip.require_cuda(obs, require)
        y_rows = obs.reshape(max(view.batch_size, 1),
                             *(operator.y_shape if y_shape is None else y_shape))
        step = make_step(net, y_rows.to(torch.float32))
        if seed is None and noise_fn is None and rng == "philox":
            seed = draw_seed()
        seed = int(seed or 0)
        x = initial_sample(view.flat_shape, net.device, rng=rng, seed=seed,
                           sample_offset=sample_offset, noise_fn=noise_fn)
        ts = host_timesteps(net)

        def loop(callback=None):
            run_steps(step, x, ts, (ts[0],) if anchored else (), rng=rng, seed=seed,
                      noise_fn=noise_fn, sample_offset=sample_offset, callback=callback)

        if advance is None:
            loop()
        else:
            advance(step, x, ts, seed, loop)
        x0 = step.predict_x0(x, ts[1])
        if finish is not None:
            return finish(x0)
        x0 = view.unflatten(x0)
        if num_reconstructions == 1 and not keep_reconstruction_dim:
            x0 = x0.squeeze(len(batch_shape))
        return sampler._as_output(x0)
    finally:
        net.clear_condition()
        net.clear_sampling_parameters()
