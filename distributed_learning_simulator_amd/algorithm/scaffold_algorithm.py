"""SCAFFOLD (Karimireddy et al. 2020, "SCAFFOLD: stochastic controlled averaging for federated
learning"), server side. Not in the reference.

θ is aggregated exactly as `FedAVGAlgorithm` does (dataset-size weights, the same fp64
accumulator and all-reduce). Next to it the clients' control-variate changes Δc_i
(`msg.extra["delta_c"]`, `worker.drift_worker.ScaffoldWorker`) are added by `fl.weighted_sum` with
unit weights into a second fp64 [P] accumulator, all-reduced over the ranks alongside the first;
then c ← c + Σ Δc_i / N with N = `worker_number` (all clients, not only the selected ones), the
sum in fp64 and cast to fp32 once. c is replicated on every rank and part of the checkpoint.
"""

from __future__ import annotations

import torch

from ..message import CohortMessage, FlatParameterMessage
from ..ops import fl
from .fed_avg_algorithm import FedAVGAlgorithm


class ScaffoldAlgorithm(FedAVGAlgorithm):
    def __init__(self) -> None:
        super().__init__()
        self._c: torch.Tensor | None = None  # [P] fp32 server control variate
        self._acc_c: torch.Tensor | None = None  # [P] fp64 Σ Δc_i of the round

    def variate(self) -> torch.Tensor:
        if self._c is None:
            self._c = torch.zeros(self.layout.padded_size, dtype=torch.float32, device=self.device)
        return self._c

    def state_dict(self) -> dict:
        return {"c": self.variate().cpu()}

    def load_state_dict(self, state: dict) -> None:
        if "c" in state:
            self._c = state["c"].to(self.device)

    def _ensure_acc(self) -> None:
        super()._ensure_acc()
        if self._acc_c is None:
            self._acc_c = torch.zeros(self.layout.padded_size, dtype=torch.float64, device=self.device)

    def _process(self, msg: CohortMessage, old_parameter) -> None:
        super()._process(msg, old_parameter)
        dc = msg.extra["delta_c"]
        fl.weighted_sum(dc, torch.ones(dc.shape[0], dtype=torch.float64, device=dc.device), self._acc_c)

    def _reduce(self) -> None:
        super()._reduce()
        self.comm.all_reduce_(self._acc_c)

    def aggregate_worker_data(self, old_parameter: torch.Tensor) -> FlatParameterMessage:
        self._ensure_acc()
        msg = super().aggregate_worker_data(old_parameter)  # (reduces both accumulators)
        n = float(self.config.worker_number)
        self._c = (self.variate().double() + self._acc_c / n).float()
        self._acc_c = None
        return msg

    def clear_worker_data(self) -> None:
        super().clear_worker_data()
        self._acc_c = None
