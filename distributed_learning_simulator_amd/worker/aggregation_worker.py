"""FedAvg-family client cohort.

Reference `worker/aggregation_worker.py:16-144`: defaults `send_parameter_diff=True`,
`reuse_learning_rate=False`; `_get_sent_data` uploads Δ = θ − θ_g (or θ) with
`dataset_size`; `_load_result_from_server` loads the broadcast model (optimizer state reset
unless `reuse_learning_rate`, `util/model.py:6-23`); a `None` broadcast means "not selected
this round" (fixed B1: the client just skips the round).

Cohort execution: clients of this rank are processed in waves of at most `capacity` rows;
each wave = load θ_g into K rows (one broadcast launch) → lock-step local training →
Δ rows computed IN PLACE in the parameter buffer (one launch) → `endpoint.send` (wire
format + byte accounting) → yielded to the server replica before the next wave reuses the
buffers.
"""

from __future__ import annotations

from typing import Iterator

import torch

from ..engine.hooks import ExecutorHookPoint
from ..message import CohortMessage, attach_payload
from ..ops import fl
from ..options import OPTIONS
from .worker import Worker


class AggregationWorker(Worker):
    def __init__(self, config, endpoint, session=None, **kwargs):
        super().__init__(config, endpoint, session, **kwargs)
        self._send_parameter_diff = True
        self._reuse_learning_rate = False
        self._keep_optimizer_state = False
        self._epochs = config.epoch
        # IID sampling ⇒ upload the best-validation model of the round (reference
        # `aggregation_worker.py:28-29,60-67,82-86`, KeepModelHook(keep_best_model=True))
        self._choose_model_by_validation = False
        self._best_theta: torch.Tensor | None = None
        self._best_acc: torch.Tensor | None = None
        if session is not None and config.dataset_sampling == "iid" and session.dc.validation_indices is not None:
            self.enable_choose_model_by_validation()
        # `distribute_init_parameters: false` (reference aggregation_server.py:58,
        # aggregation_worker.py:36): no θ0 broadcast — in the first round every client starts
        # from its OWN random init (seeded by client id, so every rank agrees) and uploads full
        # parameters (there is no common base to take a delta against)
        self._own_init = not bool(getattr(config, "distribute_init_parameters", True))

    # ------------------------------------------------- keep best by validation
    def enable_choose_model_by_validation(self) -> None:
        self._choose_model_by_validation = True

    def disable_choose_model_by_validation(self) -> None:
        self._choose_model_by_validation = False
        self._best_theta = None
        self._best_acc = None

    def _validation_shards(self, wave: list[int]) -> list[torch.Tensor]:
        key = self.session.dc.spec.name + "/validation"
        return [self.session.practitioners[c].indices(key) for c in wave]

    def _keep_best_hook(self, wave: list[int]):
        K = len(wave)
        shards = self._validation_shards(wave)
        P = self.trainer.buffers.theta.shape[1]
        if self._best_theta is None or self._best_theta.shape[0] < K:
            self._best_theta = torch.empty((self.trainer.capacity, P), dtype=torch.float32,
                                           device=self.trainer.buffers.theta.device)
        self._best_acc = torch.full((K,), -1.0, device=self._best_theta.device)

        def after_epoch(**_):
            acc = self.trainer.evaluate_clients(K, shards)
            better = acc > self._best_acc
            self._best_acc = torch.where(better, acc, self._best_acc)
            theta = self.trainer.buffers.theta[:K]
            self._best_theta[:K].copy_(torch.where(better[:, None], theta, self._best_theta[:K]))

        return after_epoch

    # ------------------------------------------------------------ round driver
    def local_epochs(self) -> int:
        return self._epochs

    def upload_kind(self) -> str:
        return "delta" if (self._send_parameter_diff and not self._own_init) else "parameter"

    def run_round(self, round_num: int, theta_g: torch.Tensor, client_ids: list[int]) -> Iterator[CohortMessage]:
        self._round_num = round_num
        self.hosted(client_ids)
        cap = self.trainer.capacity
        if OPTIONS.ragged_steps:
            # cohort rows by descending shard size: in every step the clients that still have a
            # batch are a row prefix, so a ragged step runs only those rows (CohortTrainer)
            name = self.session.dc.spec.name
            client_ids = sorted(client_ids, key=lambda c: (-self.session.practitioners[c].dataset_size(name), c))
        for w0 in range(0, len(client_ids), cap):
            wave = client_ids[w0 : w0 + cap]
            yield self.train_wave(round_num, theta_g, wave)
        self._own_init = False  # from round 2 on every client starts from the broadcast model

    def train_wave(self, round_num: int, theta_g: torch.Tensor, wave: list[int]) -> CohortMessage:
        K = len(wave)
        if self._own_init:
            self._load_own_init(wave)
        else:
            self._load_result_from_server(theta_g, K)
        schedule = self.build_schedule(round_num, wave)
        if self._choose_model_by_validation:
            self.trainer.hooks.append_named_hook(ExecutorHookPoint.AFTER_EPOCH, "keep_model_hook",
                                                 self._keep_best_hook(wave))
        try:
            stats = self.trainer.train(schedule, executor=self)
        finally:
            self.trainer.hooks.remove_named_hook("keep_model_hook")
        self.log_train_stats(wave, stats, len(schedule.epoch_end) - 1)
        msg = self._get_sent_data(wave, theta_g, stats)
        return self.endpoint.send(msg, seed=self.upload_seed(round_num))

    def build_schedule(self, round_num: int, wave: list[int]):
        return self.trainer.build_schedule(
            self.shards(wave), self.local_epochs(),
            seed=self.config.seed * 100_003 + round_num * 1009, client_ids=list(wave),
        )

    def upload_seed(self, round_num: int) -> int:
        return (self.config.seed * 7_368_787 + round_num * 104_729) & 0x7FFFFFFF

    # -------------------------------------------------------------- hooks
    def _load_result_from_server(self, theta_g: torch.Tensor, K: int) -> None:
        self.trainer.load_global(theta_g, K)
        if not self._keep_optimizer_state:
            # torch semantics: fresh optimizer => momentum buffer re-initialised with the first
            # gradient (first-step flags in the schedule); Adam moments zeroed
            self.trainer.reset_optimizer(K)

    def _load_own_init(self, wave: list[int]) -> None:
        layout = self.trainer.layout
        rows = torch.stack([layout.init_flat(torch.Generator().manual_seed(
            (self.config.seed * 1_000_003 + 7919 * (c + 1)) & 0x7FFFFFFF)) for c in wave])
        self.trainer.load_rows(rows.to(self.trainer.device))
        self.trainer.reset_optimizer(len(wave))

    def _get_sent_data(self, wave: list[int], theta_g: torch.Tensor, stats) -> CohortMessage:
        K = len(wave)
        rows = self.trainer.buffers.theta[:K]
        if self._choose_model_by_validation and self._best_acc is not None:
            rows.copy_(self._best_theta[:K])  # "use best model"
        if self.upload_kind() == "delta":
            data = fl.delta_rows(rows, theta_g, out=rows)
            kind = "delta"
        else:
            data = rows
            kind = "parameter"
        return CohortMessage(client_ids=list(wave), dataset_sizes=self.dataset_sizes(wave).to(rows.device),
                             kind=kind, data=data, layout=self.trainer.layout)

    @staticmethod
    def _attach_payload(msg: CohortMessage, payload, wire_bytes: list[int], decode_into: bool = True) -> CohortMessage:
        """The wave's upload is a payload packed on the sender's side (`message.attach_payload`), which
        states its own wire bytes per client (`ClientEndpoint._dense_wire`)."""
        attach_payload(msg, payload, decode_into)
        msg.extra["wire_bytes"] = wire_bytes
        return msg
