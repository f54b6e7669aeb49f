"""The shared round skeleton of the aggregation algorithms (algorithm/aggregation_algorithm.py) and the
cohort-size rule (config.clients_per_round)."""

import pytest

from distributed_learning_simulator_amd.algorithm.aggregation_algorithm import AggregationAlgorithm
from distributed_learning_simulator_amd.algorithm.dp_algorithm import DPFedAvgAlgorithm
from distributed_learning_simulator_amd.algorithm.fed_avg_algorithm import FedAVGAlgorithm
from distributed_learning_simulator_amd.algorithm.krum_algorithm import KrumAlgorithm, MultiKrumAlgorithm
from distributed_learning_simulator_amd.algorithm.robust_algorithm import MedianAlgorithm, TrimmedMeanAlgorithm
from distributed_learning_simulator_amd.algorithm.secagg_algorithm import SecAggAlgorithm
from distributed_learning_simulator_amd.config import clients_per_round
from distributed_learning_simulator_amd.method.fed_dropout_avg import FedDropoutAvgAlgorithm

SKELETON_USERS = [FedAVGAlgorithm, TrimmedMeanAlgorithm, MedianAlgorithm, MultiKrumAlgorithm, KrumAlgorithm,
                  DPFedAvgAlgorithm, SecAggAlgorithm, FedDropoutAvgAlgorithm]

W = 8
ABSENT = object()


# expected: what the spelled-out rule gave at each of its former sites (session, DP-FedAvg's denominator,
# fed_secagg's cohort size, the analysis; the error-feedback and SCAFFOLD workers only compared it with W)
@pytest.mark.parametrize("m,expected", [(ABSENT, 8), (None, 8), (0, 8), (3, 3), (W, 8), (W + 5, 8)])
def test_clients_per_round(m, expected):
    kwargs = {} if m is ABSENT else {"random_client_number": m}
    got = clients_per_round(kwargs, W)
    assert got == expected and type(got) is int
    assert (got >= W) == (m in (ABSENT, None, 0) or m >= W)  # the workers' "full participation" test


@pytest.mark.parametrize("cls", SKELETON_USERS)
def test_algorithms_share_the_round_skeleton(cls):
    assert "aggregate_worker_data" not in cls.__dict__
    assert cls.aggregate_worker_data is AggregationAlgorithm.aggregate_worker_data
    alg = cls()
    assert alg.last_fp64 is None and alg.round_stats == {}
