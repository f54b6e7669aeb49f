"""Krum (Blanchard et al. 2017): the round's update is the ONE upload whose summed squared distance
to its n − f − 2 nearest other uploads is smallest (`algorithm/krum_algorithm.py`, distances by
csrc/krum.hip). f = `algorithm_kwargs.krum_f`, default `byzantine_number`. Not in the reference.
Byzantine clients can be injected as in `fed_trimmed_mean`."""

from ...algorithm.krum_algorithm import KrumAlgorithm
from ...server.aggregation_server import AggregationServer
from ...worker.robust_worker import ByzantineWorker
from ..algorithm_factory import CentralizedAlgorithmFactory

CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_krum",
    client_cls=ByzantineWorker,
    server_cls=AggregationServer,
    algorithm_cls=KrumAlgorithm,
)
