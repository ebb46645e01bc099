"""Host: the surface of the ViT sliding-window route -- the four C entries resolve in the built library, and
``sliding_window_volume`` refuses a host tensor before it touches the device."""
import pytest
import torch

from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2
from anatomix_amd.registration.sliding_window import sliding_window_volume
from oracle import vit_ref as V

NEW = ("amx_vit_windows_workspace_bytes", "amx_vit_forward_windows", "amx_vit_sliding_window_workspace_bytes", "amx_vit_sliding_window")


def test_the_new_symbols_resolve_in_the_built_library():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SYMBOLS[name][1] and fn.restype == _lib.SYMBOLS[name][0]
    # a null handle needs no workspace and no device
    assert lib.amx_vit_windows_workspace_bytes(None, 4) == 0 and lib.amx_vit_sliding_window_workspace_bytes(None, 4) == 0


def test_a_host_tensor_is_refused_with_the_reason():
    model = PrimusV2(**dict(V.VIT_VARIANTS["anatomix-dev-vit"], input_shape=(32, 32, 32), eva_depth=1)).eval()
    with torch.no_grad():
        with pytest.raises(_lib.AmxEnvelopeError, match="no host path"):
            sliding_window_volume(torch.zeros(1, 1, 32, 32, 32), 32, model)
    assert model._handle is None                  # refused before an engine was created
