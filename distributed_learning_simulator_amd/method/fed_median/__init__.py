"""Coordinate-wise median aggregation (Yin et al. 2018): per parameter the median of the n uploads
(the mean of the two middle values for even n), i.e. the trimmed mean with b = (n − 1) // 2
(`algorithm/robust_algorithm.py`, kernel csrc/robust.hip). Not in the reference. Byzantine clients
can be injected as in `fed_trimmed_mean`."""

from ...algorithm.robust_algorithm import MedianAlgorithm
from ...server.aggregation_server import AggregationServer
from ...worker.robust_worker import ByzantineWorker
from ..algorithm_factory import CentralizedAlgorithmFactory

CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_median",
    client_cls=ByzantineWorker,
    server_cls=AggregationServer,
    algorithm_cls=MedianAlgorithm,
)
