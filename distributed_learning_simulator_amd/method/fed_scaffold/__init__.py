"""SCAFFOLD (Karimireddy et al. 2020): every local SGD step runs on g + (c − c_i), the server's
control variate minus the client's (`ops.fl.sgd_step_corrected`, csrc/elementwise.hip); the clients
update c_i by option II of the paper and upload Δc_i with Δθ_i
(`worker.drift_worker.ScaffoldWorker`), the server averages θ as FedAvg and moves c by Σ Δc_i / N
(`algorithm.scaffold_algorithm`). Both directions carry a model and a variate: twice FedAvg's
bytes. Not in the reference."""

from ...algorithm.scaffold_algorithm import ScaffoldAlgorithm
from ...server.aggregation_server import AggregationServer
from ...topology.endpoints import ClientEndpoint, ServerEndpoint
from ...worker.drift_worker import ScaffoldWorker
from ..algorithm_factory import CentralizedAlgorithmFactory


class ScaffoldServerEndpoint(ServerEndpoint):
    """The broadcast carries θ_g and c."""

    def encode_broadcast(self, params, seed):
        return params, 2 * self.ctx.dense_bytes


CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_scaffold",
    client_cls=ScaffoldWorker,
    server_cls=AggregationServer,
    client_endpoint_cls=ClientEndpoint,
    server_endpoint_cls=ScaffoldServerEndpoint,
    algorithm_cls=ScaffoldAlgorithm,
)
