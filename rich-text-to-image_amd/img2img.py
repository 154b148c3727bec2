"""Starting a pass from an existing image (both pipelines): the pieces the two facades share.  The reference has no such path (its
loops start from noise; `inject_background` only approximates it, for images the reference generated itself).

  image        [1,3,H,W] pixels in [0,1] (encoded with the pipeline's `encode_imgs`) or [1,4,h,w] latents, taken as given
  strength     share of the schedule that is executed (schedulers.py `set_timesteps(n, strength)`)
  noise        [1,4,h,w]; the start latents are a*x0 + b*noise at the scheduler's start_level()
  keep_source  None | "background" (the region of the unformatted text, model.masks[-1][:, :1]) | [h,w] / [1,1,h,w] in [0,1]:
               after every iteration the kept pixels are reset to the source at the level the iteration reached (rt_source_blend)
"""
import torch


def latent_shape(image):
    """(h, w) of the latents `image` stands for."""
    if image.dim() != 4 or image.shape[0] != 1 or image.shape[1] not in (3, 4):
        raise ValueError(f"image: expected [1,3,H,W] pixels or [1,4,h,w] latents, got {tuple(image.shape)}")
    if image.shape[1] == 4:
        return int(image.shape[2]), int(image.shape[3])
    if image.shape[2] % 8 or image.shape[3] % 8:
        raise ValueError(f"image: height and width must be multiples of 8, got {tuple(image.shape[2:])}")
    return int(image.shape[2]) // 8, int(image.shape[3]) // 8


def source_latents(model, image):
    """x0 [1,4,h,w] fp32 on the model's device: pixels go through model.encode_imgs, latents are taken as given (no scaling)."""
    latent_shape(image)
    image = image.to(model.device).float()
    return image if image.shape[1] == 4 else model.encode_imgs(image).float()


def check_start(image, latents):
    if image is not None and latents is not None:
        raise ValueError("pass either `image` (start from an encoded image) or `latents` (start from noise), not both")


def keep_mask(model, keep_source, h, w):
    """The [h,w] fp32 keep mask of `keep_source`, or None."""
    if keep_source is None:
        return None
    if getattr(model, "split_image", False):
        raise ValueError("keep_source is not supported with split_image")
    if isinstance(keep_source, str):
        if keep_source != "background":
            raise ValueError(f"keep_source: expected None, 'background' or a tensor, got {keep_source!r}")
        if not model.masks:
            raise ValueError("keep_source='background' needs the region masks (model.masks)")
        keep_source = model.masks[-1][:, :1].clamp(0, 1)
    k = keep_source.to(model.device).float()
    if k.numel() != h * w or tuple(k.shape[-2:]) != (h, w):
        raise ValueError(f"keep_source: expected [{h},{w}] or [1,1,{h},{w}], got {tuple(k.shape)}")
    if float(k.min()) < 0.0 or float(k.max()) > 1.0:
        raise ValueError("keep_source: values must lie in [0, 1]")
    return k.reshape(h, w).contiguous()


def check_tokenmap_iterations(hooks, n_iter):
    """The hooks record from a module's 11th call on (rd.py:422, xl.py:988): a truncated loop of <= 10 iterations would hand the caller
    empty maps later."""
    if hooks and n_iter <= 10:
        raise ValueError(f"token-map hooks are registered but the executed loop has {n_iter} iterations: the maps are recorded after the "
                         "10th call only; raise num_inference_steps or strength")
