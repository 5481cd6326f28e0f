"""Host logic of fit_channels (no GPU): which images run through an RGB network as colour (+ alpha) planes, the shapes and dtypes that come back,
the refusal of other image types, and the `-fit_channels` flag."""
import numpy as np
import pytest


def test_which_images_qualify():
    from innfer_amd.utils.utils import fit_channels_plan as plan
    u8, u16 = np.uint8, np.uint16
    assert plan((10, 12), u8, 3, 3) == 1                       # gray H x W
    assert plan((10, 12, 1), u8, 3, 3) == 1                    # gray H x W x 1
    assert plan((10, 12, 2), u16, 3, 3) == 2                   # gray + alpha
    assert plan((10, 12, 4), u8, 3, 3) == 4                    # BGRA
    assert plan((10, 12), u16, 1, 1) == 0                      # 2-D image, 1-channel network: runs as H x W x 1
    assert plan((10, 12), u8, 1, 3) == 0
    # everything else goes the way it goes without the switch
    assert plan((10, 12, 3), u8, 3, 3) is None                 # already RGB
    assert plan((10, 12, 4), u8, 4, 4) is None                 # a 4-channel network takes BGRA as it is
    assert plan((10, 12, 1), u8, 1, 1) is None
    assert plan((10, 12, 4), u8, 1, 1) is None
    assert plan((10, 12, 4), u8, 3, 1) is None                 # not 3 -> 3
    assert plan((10, 12, 5), u8, 3, 3) is None
    assert plan((10, 12, 2, 1), u8, 3, 3) is None


def test_other_image_types_are_refused():
    from innfer_amd.utils.utils import fit_channels_plan as plan
    for dt in (np.float32, np.int8, np.uint32):
        with pytest.raises(NotImplementedError, match="uint8 / uint16 images"):
            plan((10, 12, 4), dt, 3, 3)
    assert plan((10, 12, 3), np.float32, 3, 3) is None         # a non-qualifying image is not checked here: its own path decides


def test_output_shapes_and_dtypes():
    from innfer_amd.utils.utils import fit_channels_out_shape as shape
    assert shape((10, 12), 4) == (40, 48)
    assert shape((10, 12, 1), 2) == (20, 24, 1)
    assert shape((10, 12, 2), 1) == (10, 12, 2)
    assert shape((10, 12, 4), 2) == (20, 24, 4)


def test_tensor_path_refuses_other_layouts():
    import torch
    from innfer_amd.utils import utils as U
    with pytest.raises(ValueError, match="no fit_channels layout"):
        U.fit_channels_forward(lambda t: t, np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(TypeError):
        U.fit_channels_forward(lambda t: t, torch.zeros(8, 8, 4, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        U.fit_channels_forward(lambda t: t, np.zeros((8, 8, 4), np.float32))


def test_flag_is_off_by_default():
    from innfer_amd import run as R
    assert "fit_channels" not in vars(R.build_parser().parse_args(["-m", "m.pth"]))
    assert vars(R.build_parser().parse_args(["-m", "m.pth", "-fit_channels"]))["fit_channels"] is True
