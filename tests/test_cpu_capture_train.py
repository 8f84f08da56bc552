"""CPU-side checks of captured fine-tuning steps: the device-slope entries are declared and bound, CapturedTrainStep
rejects host tensors and non-capturable optimizers before any device work, and the few-shot helpers exist under the
reference's names."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_slope_entries_declared_and_bound():
    from ragraph_amd import _native as N
    from ragraph_amd import kernels as K

    hdr = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    for name in ("ragraph_spmm_csr_prelu_dev_f32", "ragraph_act_grad_prelu_dev_f32"):
        assert f"int {name}(" in hdr
        assert name in N.SIGNATURES
    assert len(N.SIGNATURES["ragraph_spmm_csr_prelu_dev_f32"][1]) == 14
    assert len(N.SIGNATURES["ragraph_act_grad_prelu_dev_f32"][1]) == 7
    assert callable(K.spmm_csr_prelu_dev) and callable(K.act_grad_prelu_dev)


def test_device_slope_wrappers_reject_host_tensors():
    from ragraph_amd import kernels as K

    with pytest.raises(K.RagraphNativeError):
        K.act_grad_prelu_dev(torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(1))


def test_captured_train_step_rejects_host_inputs_and_non_capturable_optimizer():
    from ragraph_amd.capture import CapturedTrainStep

    lin = torch.nn.Linear(4, 2)
    calls = []

    def step(x):
        calls.append(1)
        return lin(x).sum()

    with pytest.raises(ValueError, match="ROCm device tensors"):
        CapturedTrainStep(step, torch.optim.Adam(lin.parameters(), capturable=True), torch.zeros(3, 4))
    with pytest.raises(ValueError, match="ROCm device tensors"):
        CapturedTrainStep(step, torch.optim.Adam(lin.parameters(), capturable=True))
    with pytest.raises(ValueError, match="capturable"):
        CapturedTrainStep(step, torch.optim.Adam(lin.parameters()), _FakeDeviceTensor())
    with pytest.raises(ValueError, match="capturable"):
        CapturedTrainStep(step, torch.optim.SGD(lin.parameters(), lr=0.1), _FakeDeviceTensor())
    assert not calls, "nothing may run before the checks"


class _FakeDeviceTensor(torch.Tensor):
    """A host tensor that claims to live on the device: the optimizer check must come before any use of it."""

    @staticmethod
    def __new__(cls):
        return torch.Tensor._make_subclass(cls, torch.zeros(3, 4))

    @property
    def is_cuda(self):
        return True


def test_fewshot_helpers_exported():
    import ragraph_amd.ragraph_utils as U

    for name in ("fewshot_mean_logits", "fewshot_predict_logits", "fewshot_predict_labels_by_mean"):
        assert callable(getattr(U, name))
    with pytest.raises(Exception):
        U.fewshot_mean_logits(torch.zeros(3, 4), torch.tensor([0, 1, 0]), num_class=2)   # host tensors: no fallback
