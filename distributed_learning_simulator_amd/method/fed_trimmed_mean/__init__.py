"""Coordinate-wise trimmed-mean aggregation (Yin et al. 2018): per parameter the
b = ⌊trim_ratio · n⌋ lowest and highest of the n uploads are dropped and the rest averaged,
unweighted (`algorithm/robust_algorithm.py`, kernel csrc/robust.hip). Not in the reference. The
worker can inject Byzantine clients (`worker/robust_worker.py`: `byzantine_number`,
`byzantine_attack`, `byzantine_scale`) for the aggregator to be robust against."""

from ...algorithm.robust_algorithm import TrimmedMeanAlgorithm
from ...server.aggregation_server import AggregationServer
from ...worker.robust_worker import ByzantineWorker
from ..algorithm_factory import CentralizedAlgorithmFactory

CentralizedAlgorithmFactory.register_algorithm(
    algorithm_name="fed_trimmed_mean",
    client_cls=ByzantineWorker,
    server_cls=AggregationServer,
    algorithm_cls=TrimmedMeanAlgorithm,
)
