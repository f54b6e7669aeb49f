#!/bin/bash
# One-round smoke run of every method family through the CLI (counterpart of the reference's
# test.sh / other_method_test.sh). Runs on the GPU when one is visible, else on the CPU.
# Multi-GPU: prefix each line with `python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1`.
set -e
cd "$(dirname "$0")/../.."
S="python3 ./simulator.py"
# CV
$S --config-name fed_avg/mnist.yaml ++fed_avg.round=1 ++fed_avg.epoch=1 ++fed_avg.worker_number=2 ++fed_avg.debug=True
# NLP
$S --config-name fed_avg/imdb.yaml ++fed_avg.round=1 ++fed_avg.epoch=1 ++fed_avg.worker_number=2 ++fed_avg.dataset_kwargs.scale=0.02
# Graph
$S --config-name fed_gnn/cs.yaml ++fed_gnn.round=1 ++fed_gnn.epoch=1 ++fed_gnn.worker_number=2
# GTG-Shapley
$S --config-name gtg_sv/mnist.yaml ++gtg_sv.round=1 ++gtg_sv.epoch=1 ++gtg_sv.worker_number=2
# FedOBD (two-phase, NNADQ)
$S --config-name fed_obd/cifar10.yaml ++fed_obd.round=1 ++fed_obd.epoch=1 ++fed_obd.worker_number=10 \
   ++fed_obd.algorithm_kwargs.random_client_number=10 ++fed_obd.algorithm_kwargs.second_phase_epoch=1
# FedDropoutAvg / FedPAQ with partial participation
$S --config-name fed_dropout_avg/cifar100.yaml ++fed_dropout_avg.round=1 ++fed_dropout_avg.epoch=1 \
   ++fed_dropout_avg.worker_number=2 ++fed_dropout_avg.algorithm_kwargs.random_client_number=2
$S --config-name fed_paq/cifar100.yaml ++fed_paq.round=1 ++fed_paq.epoch=1 ++fed_paq.worker_number=2 \
   ++fed_paq.algorithm_kwargs.random_client_number=2
# top-k sparsified uploads with error feedback (packed payload)
$S --config-name fed_topk/mnist.yaml ++fed_topk.round=1 ++fed_topk.epoch=1 ++fed_topk.worker_number=2
# 1-bit rotated uploads (DRIVE: Hadamard rotation + sign bits): unbiased, then with error feedback
$S --config-name fed_drive/mnist.yaml ++fed_drive.round=1 ++fed_drive.epoch=1 ++fed_drive.worker_number=2
$S --config-name fed_drive/mnist.yaml ++fed_drive.round=2 ++fed_drive.epoch=1 ++fed_drive.worker_number=2 \
   ++fed_drive.algorithm_kwargs.error_feedback=true
# robust aggregation (coordinate-wise trimmed mean / median) with Byzantine clients
$S --config-name fed_trimmed_mean/mnist.yaml ++fed_trimmed_mean.round=1 ++fed_trimmed_mean.epoch=1 ++fed_trimmed_mean.worker_number=5 \
   ++fed_trimmed_mean.algorithm_kwargs.byzantine_number=1 ++fed_trimmed_mean.debug=True
$S --config-name fed_median/mnist.yaml ++fed_median.round=1 ++fed_median.epoch=1 ++fed_median.worker_number=5 \
   ++fed_median.algorithm_kwargs.byzantine_number=1 ++fed_median.algorithm_kwargs.byzantine_attack=nan ++fed_median.debug=True
# Krum / Multi-Krum (whole uploads chosen by their pairwise distances) with Byzantine clients
$S --config-name fed_krum/mnist.yaml ++fed_krum.round=1 ++fed_krum.epoch=1 ++fed_krum.worker_number=5 \
   ++fed_krum.algorithm_kwargs.byzantine_number=1 ++fed_krum.debug=True
$S --config-name fed_multi_krum/mnist.yaml ++fed_multi_krum.round=1 ++fed_multi_krum.epoch=1 ++fed_multi_krum.worker_number=5 \
   ++fed_multi_krum.algorithm_kwargs.byzantine_number=1 ++fed_multi_krum.algorithm_kwargs.byzantine_attack=nan ++fed_multi_krum.debug=True
# client-drift corrections on non-IID shards: FedProx (proximal term) and SCAFFOLD (control variates);
# two rounds, so that SCAFFOLD's second round steps on non-zero variates
$S --config-name fed_prox/mnist.yaml ++fed_prox.round=2 ++fed_prox.epoch=1 ++fed_prox.worker_number=4 ++fed_prox.debug=True
$S --config-name fed_scaffold/mnist.yaml ++fed_scaffold.round=2 ++fed_scaffold.epoch=1 ++fed_scaffold.worker_number=4 \
   ++fed_scaffold.debug=True
$S --config-name fed_dp_avg/mnist.yaml ++fed_dp_avg.round=2 ++fed_dp_avg.epoch=1 ++fed_dp_avg.worker_number=4 \
   ++fed_dp_avg.algorithm_kwargs.dp_clip_norm=0.05 ++fed_dp_avg.debug=True
# server optimisers on the aggregated pseudo-gradient (FedAvgM, FedAdagrad, FedAdam, FedYogi); two rounds,
# so that the second steps on non-zero state; and the same stage behind another aggregator
for M in fed_avgm fed_adagrad fed_adam fed_yogi; do
  $S --config-name $M/mnist.yaml ++$M.round=2 ++$M.epoch=1 ++$M.worker_number=4 ++$M.debug=True
done
$S --config-name fed_median/mnist.yaml ++fed_median.round=2 ++fed_median.epoch=1 ++fed_median.worker_number=4 \
   ++fed_median.algorithm_kwargs.server_optimizer=adam ++fed_median.debug=True
# secure aggregation (pairwise masks in Z_2^32): the complete graph, then a ring of degree 2 with a dropout
# whose masks the server rebuilds from one share
$S --config-name fed_secagg/mnist.yaml ++fed_secagg.round=2 ++fed_secagg.epoch=1 ++fed_secagg.worker_number=4 \
   ++fed_secagg.debug=True
$S --config-name fed_secagg/mnist.yaml ++fed_secagg.round=2 ++fed_secagg.epoch=1 ++fed_secagg.worker_number=6 \
   ++fed_secagg.algorithm_kwargs.secagg_degree=2 ++fed_secagg.algorithm_kwargs.secagg_threshold=1 \
   ++fed_secagg.algorithm_kwargs.failure_rate=0.2 ++fed_secagg.debug=True
# ResNet-18 with GroupNorm in place of BatchNorm (model_kwargs.norm: group) on non-IID shards, under
# FedAvg and under a server optimiser (FedAdam, two rounds so that the second steps on non-zero state)
$S --config-name fed_avg/cifar10_gn.yaml ++fed_avg.round=1 ++fed_avg.epoch=1 ++fed_avg.worker_number=4 \
   ++fed_avg.dataset_kwargs.scale=0.01 ++fed_avg.debug=True
$S --config-name fed_adam/cifar10_gn.yaml ++fed_adam.round=2 ++fed_adam.epoch=1 ++fed_adam.worker_number=4 \
   ++fed_adam.algorithm_kwargs.random_client_number=4 ++fed_adam.dataset_kwargs.scale=0.01 ++fed_adam.debug=True
# sign-SGD (1-bit majority vote)
$S --config-name sign_sgd/cifar10.yaml ++sign_sgd.round=1 ++sign_sgd.epoch=1 ++sign_sgd.worker_number=4
