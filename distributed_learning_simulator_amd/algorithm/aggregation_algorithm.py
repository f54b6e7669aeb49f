"""Server-side aggregation algorithm base: the round skeleton every method shares.

Reference `algorithm/aggregation_algorithm.py:9-96`: `get_ratios`, `weighted_avg` (static,
dict-of-messages form — kept for API parity and used by tests/analysis),
`process_worker_data(worker_id, worker_data, old_parameter_dict, save_dir)` (`None` ⇒
skipped worker), `aggregate_worker_data()`, `clear_worker_data()`, `exit()`.

Cohort form: `process_worker_data` receives a `CohortMessage` holding the uploads of every
client of one resident cohort (device rows), and the aggregation is a fused weighted
row-reduction followed by one all-reduce across ranks (see `FedAVGAlgorithm`).

A round, as `aggregate_worker_data` runs it for every method: θ_t → fp64 on the device,
`_aggregate(old)` → the fp64 θ_{t+1}, which stays in `last_fp64` (tests, the server optimiser),
ONE cast to the incoming dtype, the NaN assertion under `config.debug`, the
`FlatParameterMessage` with the round's `other_data` / `end_training`, `_reset_round()`.

A new method implements
* `_process(msg, old_parameter)`: take one cohort's uploads (accumulate or store them);
* `_aggregate(old)`: issue the round's collectives and return the fp64 θ_{t+1};
* `_reset_round()`: drop the round's state (extend it: call `super()._reset_round()`);
and may fill `round_stats` (merged into the session's metrics row) and `last_*` diagnostics. The
helpers here cover what must be the same on every rank: `_merge_round_flags` (end_training /
other_data), `_gather_client_values` (per-client host values), `round_index`.
"""

from __future__ import annotations

import torch

from ..message import CohortMessage, FlatParameterMessage, Message, ParameterMessage
from ..parallel.comm import get_comm
from ..utils.logging import get_logger


class AggregationAlgorithm:
    def __init__(self) -> None:
        self._skipped_workers: set[int] = set()
        self._worker_ids: list[int] = []
        self._other_data: dict = {}
        self._end_training: bool | None = None
        self._rounds_done = 0  # (round index when no server is bound: unit tests)
        self.last_fp64: torch.Tensor | None = None  # pre-cast fp64 θ_{t+1} of the last aggregation
        self.round_stats: dict = {}  # the method's own per-round figures (session metrics row)
        self.config = None
        self.layout = None
        self.device = torch.device("cpu")
        self.comm = get_comm()
        self.server = None

    def bind(self, config, layout, device, comm=None, server=None) -> None:
        self.config = config
        self.layout = layout
        self.device = torch.device(device)
        self.comm = comm or get_comm()
        self.server = server

    # --------------------------------------------------------- reference helpers
    @classmethod
    def get_ratios(cls, data_dict: dict[int, ParameterMessage], key_name: str | None = None) -> dict[int, float]:
        if key_name is None:
            total = sum(v.dataset_size for v in data_dict.values())
            return {k: float(v.dataset_size) / float(total) for k, v in data_dict.items()}
        total = sum(v.other_data[key_name] for v in data_dict.values())
        return {k: float(v.other_data[key_name]) / float(total) for k, v in data_dict.items()}

    @classmethod
    def weighted_avg(cls, data_dict: dict[int, ParameterMessage], weight_dict: dict[int, float]) -> dict:
        assert data_dict
        avg: dict[str, torch.Tensor] = {}
        for wid, v in data_dict.items():
            ratio = weight_dict[wid]
            assert 0 <= ratio <= 1
            for k, t in v.parameter.items():
                avg[k] = avg[k] + t * ratio if k in avg else t * ratio
        for t in avg.values():
            assert not t.isnan().any()
        return avg

    # ------------------------------------------------------------- cohort API
    def _check_other_data(self, msg: Message) -> None:
        """`fed_avg_algorithm.py:99-110`: other_data must agree across workers."""
        for k, v in msg.other_data.items():
            if k in self._other_data and self._other_data[k] != v:
                get_logger().error("different values on key %s", k)
                raise RuntimeError(f"different values on key {k}")
            self._other_data[k] = v
        if self._end_training is None:
            self._end_training = msg.end_training

    def process_worker_data(self, worker_data: CohortMessage | None, old_parameter: torch.Tensor | None,
                            worker_ids: list[int] | None = None, save_dir: str | None = None) -> None:
        if worker_data is None:
            self._skipped_workers.update(worker_ids or [])
            return
        self._check_other_data(worker_data)
        self._worker_ids.extend(worker_data.client_ids)
        self._process(worker_data, old_parameter)

    def _process(self, msg: CohortMessage, old_parameter) -> None:
        raise NotImplementedError

    def aggregate_worker_data(self, old_parameter: torch.Tensor) -> FlatParameterMessage:
        new = self._aggregate(old_parameter.to(self.device, torch.float64))
        self.last_fp64 = new
        new = new.to(old_parameter.dtype)
        if self.config is not None and self.config.debug:
            assert not torch.isnan(new).any(), "NaN in aggregated parameters"
        msg = FlatParameterMessage(parameter=new, layout=self.layout, other_data=dict(self._other_data),
                                   end_training=bool(self._end_training))
        self._rounds_done += 1
        self._reset_round()
        return msg

    def _aggregate(self, old: torch.Tensor) -> torch.Tensor:
        """fp64 θ_t on the device → fp64 θ_{t+1}, the same on every rank."""
        raise NotImplementedError

    def _reset_round(self) -> None:
        """Drop what `_process` collected for the round (after every aggregation, and on clear)."""

    def round_index(self) -> int:
        """The round being aggregated: the server's, or an own count when bound without a server."""
        return int(self.server.round_number) if self.server is not None else self._rounds_done + 1

    _round = round_index  # (the name DP-FedAvg and SecAgg had for it: their session tests' spies call it)

    # ------------------------------------------------------------------ ranks
    def _merge_round_flags(self, end: bool, other: bool) -> None:
        """end_training / other_data must agree on every server replica. `end`, `other`: whether any
        rank ends training / carries other_data, the two bits that rode in the caller's own small
        collective; the pickled gather runs only in a round where some rank has other_data to merge."""
        if end:
            self._end_training = True
        if other:
            for _, od in self.comm.all_gather_object((self._end_training, self._other_data)):
                for k, v in od.items():
                    self._other_data.setdefault(k, v)

    def _gather_client_values(self, ids: list[int], tensors: list[torch.Tensor]) -> dict[int, tuple]:
        """client id -> tuple of its values over all ranks, in client-id order. `tensors`: this rank's
        device tensors of the round, [k] or [k, v] each, their rows in the order of `ids`. ONE host
        read, and one `all_gather_object` when distributed."""
        local = torch.cat(tensors).tolist() if tensors else []
        rows = [(c, *v) if isinstance(v, list) else (c, v) for c, v in zip(ids, local)]
        if self.comm.is_distributed:
            rows = [r for part in self.comm.all_gather_object(rows) for r in part]
        return {r[0]: r[1:] for r in sorted(rows)}

    def clear_worker_data(self) -> None:
        self._skipped_workers.clear()
        self._worker_ids.clear()
        self._other_data = {}
        self._end_training = None
        self._reset_round()

    def exit(self) -> None:
        pass
