"""Exact t-SNE on the C++ twin (bodies: tests/tsne_forms.py; the same bodies on the GPU: tests/test_gpu_tsne.py)."""
import pytest

import tsne_forms as F

DEV = "cpu"


@pytest.mark.parametrize("n,d", F.AFFINITY_CASES)
def test_affinities(n, d):
    F.body_affinities(DEV, n, d)


@pytest.mark.parametrize("n,d", [(4, 3), (65, 131), (257, 3), (300, 16)])
def test_row_entropy_at_default_tolerance(n, d):
    F.body_entropy(DEV, n, d)


def test_affinities_against_sklearn():
    F.body_sklearn(DEV)


@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
@pytest.mark.parametrize("scale", [1e-4, 5.0])
@pytest.mark.parametrize("n", F.SIZES)
def test_gradient_and_kl(n, scale, exaggeration):
    F.body_gradient(DEV, n, scale, exaggeration)


@pytest.mark.parametrize("n", F.LARGE)
def test_gradient_second_pass(n):
    F.body_gradient_large(DEV, n)


def test_lockstep_optimisation():
    F.body_lockstep(DEV)


def test_end_to_end():
    F.body_end_to_end(DEV)


def test_end_to_end_against_sklearn():
    F.body_end_to_end(DEV, against="sklearn")


def test_repeats_are_bit_identical():
    F.body_repeat(DEV)


@pytest.mark.parametrize("n", [65, 300])
def test_step_is_gradient_then_update(n):
    F.body_step_is_gradient_then_update(DEV, n)


def test_permuted_rows():
    F.body_permutation(DEV)


def test_inits_and_learning_rate():
    F.body_inits_and_learning_rate(DEV)


def test_refusals():
    F.body_refusals(DEV)


def test_reference_gradient_is_the_derivative_of_kl():
    F.body_finite_difference()
