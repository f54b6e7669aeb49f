"""FedProx (Li et al. 2020, "Federated optimization in heterogeneous networks"): FedAvg whose local
objective carries the proximal term (μ/2)·‖θ_i − θ_g‖², i.e. every local SGD step runs on
g + μ·(θ_i − θ_g) (`ops.fl.sgd_step_corrected`, csrc/elementwise.hip). μ =
`algorithm_kwargs.proximal_mu` (default 0.01; 0 is a plain `fed_avg` run). Uploads, aggregation and
byte counts are FedAvg's. Not in the reference."""

from ...algorithm.fed_avg_algorithm import FedAVGAlgorithm
from ...server.aggregation_server import AggregationServer
from ...worker.drift_worker import FedProxWorker
from ..algorithm_factory import CentralizedAlgorithmFactory

CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_prox",
    client_cls=FedProxWorker,
    server_cls=AggregationServer,
    algorithm_cls=FedAVGAlgorithm,
)
