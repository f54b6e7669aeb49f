"""Multi-Krum (Blanchard et al. 2017): the unweighted mean of the m uploads with the smallest Krum
scores (`algorithm/krum_algorithm.py`, distances by csrc/krum.hip). m = `algorithm_kwargs.krum_m`,
default n − f; f = `algorithm_kwargs.krum_f`, default `byzantine_number`. Not in the reference.
Byzantine clients can be injected as in `fed_trimmed_mean`."""

from ...algorithm.krum_algorithm import MultiKrumAlgorithm
from ...server.aggregation_server import AggregationServer
from ...worker.robust_worker import ByzantineWorker
from ..algorithm_factory import CentralizedAlgorithmFactory

CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_multi_krum",
    client_cls=ByzantineWorker,
    server_cls=AggregationServer,
    algorithm_cls=MultiKrumAlgorithm,
)
