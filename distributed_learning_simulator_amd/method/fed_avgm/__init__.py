"""FedAvgM (Hsu et al. 2019, "Measuring the effects of non-identical data distribution for federated
visual classification"): FedAvg whose server keeps a momentum buffer over the rounds' pseudo-gradients,
m' = β1·m + d, θ' = θ + lr·m'
(`ops.fl.server_opt_step`, csrc/server_opt.hip; the stage is server/server_optimizer.py, which presets the
rule `sgdm` from this method's name). Workers, uploads, aggregation and byte counts are FedAvg's;
`algorithm_kwargs`: `server_lr`, `server_beta1`, `server_beta2`, `server_tau`. Not in the reference."""

from ...algorithm.fed_avg_algorithm import FedAVGAlgorithm
from ...server.aggregation_server import AggregationServer
from ...worker.aggregation_worker import AggregationWorker
from ..algorithm_factory import CentralizedAlgorithmFactory

CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_avgm",
    client_cls=AggregationWorker,
    server_cls=AggregationServer,
    algorithm_cls=FedAVGAlgorithm,
)
