"""fed_secagg client cohort: every upload leaves the rank as a pairwise-masked fixed-point vector.

After local training the wave's delta rows are quantised to the fixed-point code of the round and the
client's masks are added in Z_{2^32}, in place in the parameter buffer (`ops.fl.secagg_mask_rows`,
csrc/secagg.hip): one launch per wave, no new [K, P] buffer. The entry table (pair keys and signs, the self
mask seed) comes from utils/secagg_protocol.py, keyed by (seed, round) over the round's SELECTED clients. The
message carries a `MaskedPayload`; its bytes are the masked vector plus the protocol's key and share
traffic. The per-row clamp / NaN counters travel in `msg.extra["secagg_stats"]`: a real server could not see
them — they are simulator diagnostics.
"""

from __future__ import annotations

import torch

from ..algorithm.secagg_algorithm import secagg_settings
from ..message import CohortMessage
from ..ops import compress, fl
from ..topology.endpoints import QuantClientEndpoint
from ..utils.secagg_protocol import round_protocol
from .aggregation_worker import AggregationWorker


class SecAggWorker(AggregationWorker):
    def __init__(self, config, endpoint, session=None, **kwargs):
        super().__init__(config, endpoint, session, **kwargs)
        if isinstance(endpoint, QuantClientEndpoint):
            raise RuntimeError("fed_secagg: a quantising endpoint would re-encode the masked words; plain endpoints only")
        if not self._send_parameter_diff or self._own_init:
            raise RuntimeError("fed_secagg masks client deltas: distribute_init_parameters must stay on")
        self.range, self.frac_bits, self.degree, self.threshold = secagg_settings(config)

    def _selected(self) -> list[int]:
        return list(self.session.server.selected)

    def _get_sent_data(self, wave: list[int], theta_g: torch.Tensor, stats) -> CohortMessage:
        msg = super()._get_sent_data(wave, theta_g, stats)
        if msg.kind != "delta":
            raise RuntimeError(f"fed_secagg masks client deltas, got an upload of kind {msg.kind!r}")
        proto = round_protocol(self.config.seed, self._round_num, self._selected(), self.degree, self.threshold)
        rows = msg.data
        words, counters = fl.secagg_mask_rows(rows, proto.entry_table(wave), self.range, self.frac_bits,
                                              out=rows.view(torch.int32))
        wire = [proto.row_bytes(c, self.trainer.layout.num_params) for c in wave]
        msg.extra["secagg_stats"] = counters
        # (no decode target: nobody can decode a masked upload)
        return self._attach_payload(msg, compress.MaskedPayload(words, wire), wire, decode_into=False)
