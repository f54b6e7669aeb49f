"""Client-drift corrections for non-IID data: FedProx and SCAFFOLD cohorts. Not in the reference.

Both change the local optimiser step, not the upload: every local step of every resident client
runs on g' = g + (c − c_i) + μ·(θ_i − θ_g) (`ops.fl.sgd_step_corrected`, one fused kernel). The
trainer applies it as a step correction (`CohortTrainer.set_step_correction`), not through an
`OPTIMIZER_STEP` hook, so sub-cohort streams, ragged steps and HIP-graph replay stay on; the fused
weight-gradient step is off for these methods (its epilogues know nothing of g').

* `FedProxWorker` (Li et al. 2020): μ = `algorithm_kwargs.proximal_mu` (default 0.01), no variates;
  uploads, aggregation and byte counts are FedAvg's. `proximal_mu: 0` sets no correction at all.
* `ScaffoldWorker` (Karimireddy et al. 2020): μ = 0 and a control variate c_i per client, a row of
  a [worker_number, P] fp32 device buffer on the rank that trains the client (zero at the start,
  allocated at first use). Per wave the correction rows are c − c_i; after training, option II
  of the paper with the round's actual step sizes,
      c_i⁺ = (c_i − c) − (θ_i − θ_g) · inv_k,   inv_k = fl32(1 / Σ_s lr[s, k]) over k's active steps
  (the sum on the host in fp64 from the schedule), and Δc_i = c_i⁺ − c_i travels with the upload
  (`msg.extra["delta_c"]`). A client without an active step keeps c_i and sends Δc_i = 0. The
  server's c is read from `ScaffoldAlgorithm` (replicated on every rank). The variates are part of
  the checkpoint (`state_dict`); as with the error-feedback residuals, the checkpoint is written by
  rank 0 and holds that rank's rows. Partial participation on more than one rank is refused: the
  client→rank assignment would not be stable, and a variate lives on the rank that trains it.
"""

from __future__ import annotations

import torch

from ..config import clients_per_round
from ..message import CohortMessage
from ..ops import fl
from .aggregation_worker import AggregationWorker


def _needs_broadcast_model(config, name: str) -> None:
    if not bool(getattr(config, "distribute_init_parameters", True)):
        raise ValueError(f"{name} needs `distribute_init_parameters: true`: the broadcast model is the anchor of "
                         "its local steps")


class FedProxWorker(AggregationWorker):
    def __init__(self, config, endpoint, session=None, **kwargs):
        super().__init__(config, endpoint, session, **kwargs)
        mu = config.algorithm_kwargs.get("proximal_mu", 0.01)
        self.proximal_mu = 0.01 if mu is None else float(mu)
        if self.proximal_mu < 0:
            raise ValueError(f"proximal_mu must be >= 0, got {self.proximal_mu}")
        if self.proximal_mu != 0.0:
            _needs_broadcast_model(config, "fed_prox")
            if session is not None:
                self.trainer.set_step_correction(self.proximal_mu, variates=False)


class ScaffoldWorker(AggregationWorker):
    def __init__(self, config, endpoint, session=None, **kwargs):
        super().__init__(config, endpoint, session, **kwargs)
        _needs_broadcast_model(config, "fed_scaffold")
        assert self._send_parameter_diff
        sel = clients_per_round(config.algorithm_kwargs, config.worker_number)
        world = session.comm.world if session is not None else 1
        if sel < config.worker_number and world > 1:
            raise ValueError("fed_scaffold: partial participation (random_client_number < worker_number) with more "
                             "than one rank is refused: the client→rank assignment would not be stable, and a "
                             "client's control variate lives on the rank that trains it")
        # the variate update needs the FINAL θ_i of the round, not the best-by-validation one
        self.disable_choose_model_by_validation()
        self._variates: torch.Tensor | None = None  # [worker_number, P] c_i rows
        self._inv_steps: torch.Tensor | None = None  # [K] fp32 1 / Σ lr of the wave in flight (0: no step)
        if session is not None:
            self.trainer.set_step_correction(0.0, variates=True)

    def enable_choose_model_by_validation(self) -> None:
        pass  # (see __init__)

    @staticmethod
    def memory_plan(config, layout) -> tuple[int, int]:
        """(extra fp32 rows per resident client, bytes held outside the cohort buffers) for the
        session's capacity plan: the correction row (`buffers.corr`, which also carries Δc) and the
        variate update's one temporary row; the [worker_number, P] variate store."""
        return 2, int(config.worker_number) * layout.padded_size * 4

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        return {"variates": self._variates.cpu()} if self._variates is not None else {}

    def load_state_dict(self, state: dict) -> None:
        if "variates" in state:
            self._variates = state["variates"].to(self.trainer.device)

    def variates(self) -> torch.Tensor:
        if self._variates is None:
            P = self.trainer.buffers.theta.shape[1]
            self._variates = torch.zeros((self.config.worker_number, P), dtype=torch.float32,
                                         device=self.trainer.device)
        return self._variates

    def server_variate(self) -> torch.Tensor:
        return self.session.server.algorithm.variate()

    # ------------------------------------------------------------------ round
    def build_schedule(self, round_num: int, wave: list[int]):
        schedule = super().build_schedule(round_num, wave)
        total = (schedule.lr.cpu().double() * schedule.active.cpu().double()).sum(0)  # [K] fp64, host
        inv = torch.where(total > 0, 1.0 / total.clamp(min=1e-300), torch.zeros_like(total))
        self._inv_steps = inv.float().to(self.trainer.device)
        # the wave's correction rows (θ_g is already loaded: train_wave loads before it builds)
        idx = torch.tensor(wave, device=self.trainer.device)
        self.trainer.load_correction(self.server_variate().unsqueeze(0) - self.variates()[idx])
        return schedule

    def _get_sent_data(self, wave, theta_g, stats) -> CohortMessage:
        msg = super()._get_sent_data(wave, theta_g, stats)
        K = len(wave)
        assert msg.kind == "delta"
        delta = msg.data  # θ_i − θ_g
        variates = self.variates()
        idx = torch.tensor(wave, device=delta.device)
        inv = self._inv_steps
        # in the correction rows (free until the next wave loads them; the server consumes the
        # message before that), one [K, P] temporary: (c_i − c) is the rows negated (fp32
        # subtraction is antisymmetric), then − Δ·inv_k
        new = self.trainer.buffers.corr[:K]
        tmp = delta * inv[:, None]
        new.neg_().sub_(tmp)
        torch.index_select(variates, 0, idx, out=tmp)  # c_i
        torch.where((inv > 0)[:, None], new, tmp, out=new)
        variates[idx] = new
        msg.extra["delta_c"] = new.sub_(tmp)
        wire = 2 * self.trainer.layout.num_params * 4  # Δθ and Δc
        msg.extra["wire_bytes"] = [wire] * K
        return msg
