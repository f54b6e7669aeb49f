"""FedAvg with top-k sparsified uploads and error feedback (the concrete form of the reference's
abstract `worker/error_feedback_worker.py`): each client uploads the k = ⌊topk_ratio · P⌋
largest-magnitude entries of Δ + e as a packed (int32 index, fp32 value) payload — 8k bytes —
and keeps the rest as its residual e. The server's fp64 accumulation reads the payload directly
(`ops.compress.SparsePayload.accumulate`); the downlink is dense. The residual lives with the
client's rank, so the configs use full participation."""

from ...algorithm.fed_avg_algorithm import FedAVGAlgorithm
from ...server.aggregation_server import AggregationServer
from ...worker.error_feedback_worker import PackedTopKWorker
from ..algorithm_factory import CentralizedAlgorithmFactory

CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_topk",
    client_cls=PackedTopKWorker,
    server_cls=AggregationServer,
    algorithm_cls=FedAVGAlgorithm,
)
