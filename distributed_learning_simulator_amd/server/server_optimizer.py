"""Server optimisers: the aggregated model as a pseudo-gradient (Reddi et al. 2021, "Adaptive federated
optimization": FedAdagrad, FedAdam, FedYogi, Algorithm 2, no bias correction; Hsu et al. 2019: FedAvgM,
server momentum). Not in the reference.

Every dense aggregation algorithm ends a round with `target`, its fp64 result before the cast
(`algorithm.last_fp64`): the weighted mean of FedAvg, a median, a Krum selection, a clipped and noised
DP mean. Without this stage θ_{t+1} = fl32(target). With it, d = target − θ_t is the round's
pseudo-gradient and `ops.fl.server_opt_step` (csrc/server_opt.hip, oracle ops/ref.py) takes one
optimiser step on it: θ fp32 and the fp64 state m, v in one fused pass, every operation rounded once, the
same bits on both backends. Every rank holds the same `target` after the algorithm's all-reduce, so
every rank takes the same step: no new collective.

`algorithm_kwargs`: `server_optimizer` (absent / `none`: no stage; `sgdm`, `adagrad`, `adam`, `yogi`),
`server_lr` (1.0 for sgdm, else 0.01), `server_beta1` (0.9), `server_beta2` (0.99), `server_tau` (1e-3).
The methods fed_avgm / fed_adagrad / fed_adam / fed_yogi preset the rule (`METHOD_RULES`); every other
dense method takes the key. State: m = +0, v = fl64(τ·τ) (Reddi's v₋₁ ≥ τ²), fp64 [padded_size] on the
device, and a step count; all three travel in the checkpoint as plain CPU tensors / ints. A round with
no active client skips the stage: θ, m, v and the count stay as they are.
"""

from __future__ import annotations

import torch

from ..message import FlatParameterMessage
from ..ops import fl, ref

METHOD_RULES = {"fed_avgm": "sgdm", "fed_adagrad": "adagrad", "fed_adam": "adam", "fed_yogi": "yogi"}
DEFAULT_LR = {"sgdm": 1.0, "adagrad": 0.01, "adam": 0.01, "yogi": 0.01}


def server_opt_settings(config) -> tuple[str, float, float, float, float] | None:
    """(rule, lr, β1, β2, τ) from `algorithm_kwargs` and the method name, or None when the stage is
    off; ValueError on bad values and on a `server_optimizer` that contradicts the method's own rule."""
    kw = config.algorithm_kwargs
    method = str(getattr(config, "distributed_algorithm", "") or "")
    preset = METHOD_RULES.get(method)
    rule = kw.get("server_optimizer")
    rule = None if rule is None else str(rule).lower()
    if preset is not None:
        if rule is not None and rule != preset:
            raise ValueError(f"{method}: server_optimizer is {preset!r} by the method's name, got {rule!r}")
        rule = preset
    if rule is None or rule == "none":
        return None
    if rule not in ref.SERVER_OPT_RULES:
        raise ValueError(f"server_optimizer must be one of none, {', '.join(ref.SERVER_OPT_RULES)}; got {rule!r}")

    def number(key, default):
        value = kw.get(key)
        try:
            return float(default if value is None else value)
        except (TypeError, ValueError) as e:
            raise ValueError(f"{key} must be a number ({e})") from e

    lr, beta1 = number("server_lr", DEFAULT_LR[rule]), number("server_beta1", 0.9)
    beta2, tau = number("server_beta2", 0.99), number("server_tau", 1e-3)
    try:
        return ref.check_server_opt(rule, lr, beta1, beta2, tau)
    except ValueError as e:
        raise ValueError(f"server_lr / server_beta1 / server_beta2 / server_tau: {e}") from e


def state_bytes(config, layout) -> int:
    """Device bytes the stage keeps for this config: m (and v for the adaptive rules) in fp64, and the
    fp64 pre-cast result it leaves in `last_fp64`; 0 when the stage is off."""
    settings = server_opt_settings(config)
    if settings is None:
        return 0
    return (2 if settings[0] == "sgdm" else 3) * 8 * int(layout.padded_size)


class ServerOptimizer:
    def __init__(self, config) -> None:
        settings = server_opt_settings(config)
        if settings is None:
            raise ValueError("no server optimiser is configured (algorithm_kwargs.server_optimizer)")
        self.rule, self.lr, self.beta1, self.beta2, self.tau = settings
        self.method = str(getattr(config, "distributed_algorithm", "") or "")
        self.m: torch.Tensor | None = None
        self.v: torch.Tensor | None = None
        self.steps = 0
        self.last_fp64: torch.Tensor | None = None  # the pre-cast fp64 x of the last step (tests)

    @classmethod
    def from_config(cls, config) -> "ServerOptimizer | None":
        return cls(config) if server_opt_settings(config) is not None else None

    def _ensure_state(self, P: int, device) -> None:
        if self.m is None:
            self.m = torch.zeros(P, dtype=torch.float64, device=device)
            if self.rule != "sgdm":
                self.v = torch.full((P,), self.tau * self.tau, dtype=torch.float64, device=device)
        if self.m.numel() != P:
            raise RuntimeError(f"server optimiser state has {self.m.numel()} elements, the model {P}")
        if self.m.device != device:
            self.m = self.m.to(device)
            self.v = None if self.v is None else self.v.to(device)

    def step(self, theta: torch.Tensor, result, algorithm):
        """θ_t and the algorithm's finished round → the message with the stepped θ_{t+1}."""
        name = self.method or type(algorithm).__name__
        if not isinstance(result, FlatParameterMessage):
            raise RuntimeError(f"{name}: the server optimiser needs a dense aggregated model, the method's result is "
                               f"a {type(result).__name__}")
        target = getattr(algorithm, "last_fp64", None)
        P = theta.numel()
        if (not isinstance(target, torch.Tensor) or target.dtype != torch.float64 or target.dim() != 1
                or target.numel() < P):
            raise RuntimeError(f"{name}: the server optimiser needs the aggregation's fp64 result "
                               f"(`last_fp64`, fp64 [>= {P}]), which {type(algorithm).__name__} does not leave")
        if theta.dtype != torch.float32:
            raise RuntimeError(f"{name}: the server optimiser steps an fp32 global model, got {theta.dtype}")
        self._ensure_state(P, theta.device)
        new = theta.detach().clone()
        x = torch.empty(P, dtype=torch.float64, device=theta.device)
        fl.server_opt_step(new, target.to(theta.device), self.m, self.v, self.rule, self.lr, self.beta1, self.beta2,
                           self.tau, x_out=x)
        self.steps += 1
        self.last_fp64 = x
        result.parameter = new
        return result

    # ------------------------------------------------------------------ checkpoint
    def state_dict(self) -> dict:
        st = {"rule": self.rule, "steps": int(self.steps)}
        if self.m is not None:
            st["m"] = self.m.detach().cpu()
        if self.v is not None:
            st["v"] = self.v.detach().cpu()
        return st

    def load_state_dict(self, state: dict) -> None:
        if state.get("rule", self.rule) != self.rule:
            raise ValueError(f"the checkpoint holds {state.get('rule')!r} server optimiser state, the run is {self.rule!r}")
        self.steps = int(state.get("steps", 0))
        self.m = state["m"].to(torch.float64).clone() if "m" in state else None
        self.v = state["v"].to(torch.float64).clone() if "v" in state else None
