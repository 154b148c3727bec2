"""sample.py's image-start flags on the CPU: the image loader and the flag combinations that are refused before anything starts."""
import numpy as np
import pytest
import torch


def test_load_init_image_resizes_to_height_by_width(tmp_path):
    from PIL import Image
    from rich_text_to_image_amd.sample import load_init_image
    rgb = np.zeros((40, 60, 3), dtype=np.uint8)
    rgb[..., 0], rgb[:20, :, 1], rgb[:, 30:, 2] = 255, 128, 64
    Image.fromarray(rgb).save(tmp_path / "a.png")
    img = load_init_image(str(tmp_path / "a.png"), 64, 96)
    assert img.shape == (1, 3, 64, 96) and img.dtype == torch.float32 and img.is_contiguous()
    assert 0.0 <= float(img.min()) and float(img.max()) <= 1.0
    assert torch.all(img[0, 0] == 1.0) and abs(float(img[0, 1, 5, 5]) - 128 / 255) < 1e-6 and float(img[0, 1, 60, 5]) == 0.0
    same = load_init_image(str(tmp_path / "a.png"), 40, 60)
    assert torch.equal(same, torch.from_numpy(rgb.astype(np.float32) / 255).permute(2, 0, 1)[None])
    Image.fromarray(rgb[..., 0]).save(tmp_path / "grey.png")                     # any mode PIL opens is read as RGB
    assert load_init_image(str(tmp_path / "grey.png"), 16, 16).shape == (1, 3, 16, 16)


def test_flags_parse_and_bad_combinations_are_refused():
    from rich_text_to_image_amd.sample import build_parser, main
    a = build_parser().parse_args([])
    assert a.init_image is None and a.strength == 0.8 and a.keep_source == "none"
    a = build_parser().parse_args(["--init_image", "a.png", "--strength", "0.6", "--keep_source", "background"])
    assert (a.init_image, a.strength, a.keep_source) == ("a.png", 0.6, "background")
    with pytest.raises(SystemExit, match="--init_image"):
        main(["--rich_text_json", "{}", "--keep_source", "background"])
    with pytest.raises(SystemExit, match="--split_image"):
        main(["--rich_text_json", "{}", "--init_image", "a.png", "--keep_source", "background", "--split_image", "--gpus", "2"])
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--keep_source", "foreground"])
