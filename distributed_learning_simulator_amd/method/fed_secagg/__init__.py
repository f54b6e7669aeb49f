"""Secure aggregation with pairwise masks (Bonawitz et al. 2017; Bell et al. 2020): every client uploads its
delta as fixed-point words of Z_{2^32} under masks that cancel in the sum, and the server unmasks only the sum
(`worker/secagg_worker.py`, `algorithm/secagg_algorithm.py`, `utils/secagg_protocol.py`, kernels
csrc/secagg.hip). Not in the reference. A simulation of the protocol's arithmetic, failure handling and cost:
Philox is no cryptographic generator, the key agreement is a toy, all parties share one process — it gives
no security to anybody."""

from ...algorithm.secagg_algorithm import SecAggAlgorithm
from ...server.aggregation_server import AggregationServer
from ...worker.secagg_worker import SecAggWorker
from ..algorithm_factory import CentralizedAlgorithmFactory

CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_secagg",
    client_cls=SecAggWorker,
    server_cls=AggregationServer,
    algorithm_cls=SecAggAlgorithm,
)
