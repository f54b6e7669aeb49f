"""Client-level DP-FedAvg (McMahan et al. 2018): every client's delta is clipped to the L2 norm
`algorithm_kwargs.dp_clip_norm`, the clipped deltas are added unweighted, Gaussian noise of std
`dp_noise_multiplier` · `dp_clip_norm` is added to the sum and the result divided by the fixed cohort
size (`algorithm/dp_algorithm.py`, kernels csrc/dp.hip, accountant utils/privacy.py). Not in the
reference. With the noise off the clipping alone bounds what one client can move the model by, so
Byzantine clients can be injected as in `fed_trimmed_mean`."""

from ...algorithm.dp_algorithm import DPFedAvgAlgorithm
from ...server.aggregation_server import AggregationServer
from ...worker.robust_worker import ByzantineWorker
from ..algorithm_factory import CentralizedAlgorithmFactory

CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_dp_avg",
    client_cls=ByzantineWorker,
    server_cls=AggregationServer,
    algorithm_cls=DPFedAvgAlgorithm,
)
