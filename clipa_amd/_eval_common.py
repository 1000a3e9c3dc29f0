"""What the evaluators (fewshot.py, zero_shot.py, search.py) share on the host side."""
import contextlib

import torch


def unwrap_model(model):                      # zero_shot.py:22-26
    return model.module if hasattr(model, "module") else model


def _features(t, name, who, check_finite=False):
    """A feature matrix as the kernels take it: a 2-D float GPU tensor -> detached fp32.  check_finite also raises on non-finite
    values (one host sync)."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 2 or not t.dtype.is_floating_point:
        raise RuntimeError(f"clipa_amd.{who}: {name} must be a 2-D float GPU tensor (no CPU fallback); got "
                           f"{(t.device, t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
    t = t.detach().float()
    if check_finite and not bool(torch.isfinite(t).all()):
        raise RuntimeError(f"clipa_amd.{who}: {name} holds non-finite values")
    return t


@contextlib.contextmanager
def _inference(model):
    """The unwrapped model in eval mode under no_grad; its previous mode is put back on the way out."""
    m = unwrap_model(model)
    was_training = m.training
    m.eval()
    try:
        with torch.no_grad():
            yield m
    finally:
        m.train(was_training)
