"""FedAvg with 1-bit rotated uploads (DRIVE, Vargaftik et al., NeurIPS 2021; EDEN, ICML 2022): each
client rotates its delta by a randomised Hadamard transform per block of 4096 flat elements, so that
every coordinate carries about the same energy, and uploads one sign bit per coordinate plus one fp32
scale per block: 516 bytes per block instead of 16384. The server's fp64 accumulation rotates back
straight from the bits (`ops.compress.RotSignPayload.accumulate`); the downlink is dense.
`algorithm_kwargs.error_feedback: false` (default) uses DRIVE's unbiased scale and keeps no client
state; `true` uses the MSE-optimal scale with the error-feedback residual of `fed_topk`."""

from ...algorithm.fed_avg_algorithm import FedAVGAlgorithm
from ...server.aggregation_server import AggregationServer
from ...worker.error_feedback_worker import RotSignWorker
from ..algorithm_factory import CentralizedAlgorithmFactory

CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_drive",
    client_cls=RotSignWorker,
    server_cls=AggregationServer,
    algorithm_cls=FedAVGAlgorithm,
)
