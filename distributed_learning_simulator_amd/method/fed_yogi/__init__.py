"""FedYogi (Reddi et al. 2021, "Adaptive federated optimization"): FedAvg whose server runs Yogi on the
rounds' pseudo-gradients, v' = v − (1 − β2)·d²·sign(v − d²), θ' = θ + lr·m' / (sqrt(v') + τ)
(`ops.fl.server_opt_step`, csrc/server_opt.hip; the stage is server/server_optimizer.py, which presets the
rule `yogi` from this method's name). Workers, uploads, aggregation and byte counts are FedAvg's;
`algorithm_kwargs`: `server_lr`, `server_beta1`, `server_beta2`, `server_tau`. Not in the reference."""

from ...algorithm.fed_avg_algorithm import FedAVGAlgorithm
from ...server.aggregation_server import AggregationServer
from ...worker.aggregation_worker import AggregationWorker
from ..algorithm_factory import CentralizedAlgorithmFactory

CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_yogi",
    client_cls=AggregationWorker,
    server_cls=AggregationServer,
    algorithm_cls=FedAVGAlgorithm,
)
