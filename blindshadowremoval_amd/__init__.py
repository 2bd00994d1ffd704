"""MI355X-native GSC shadow-removal generator forward (drop-in for the reference's ``Generator`` /
``FSRNet.test*`` inference path).  See DESIGN.md."""
from .weights import generator_variable_shapes, init_weights  # noqa: F401

__all__ = ["Generator", "GeneratorTSM", "GeneratorRGB", "ShadowSynth", "TrainLosses", "Discriminators", "Perceptual", "ColourTail", "ColourDecoder",
           "NonLocalGrad", "BottleneckGrad", "HeadsGrad", "GreyDecoder", "ColourTrunk", "LowerTrunk", "generator_variable_shapes", "init_weights"]


def __getattr__(name):
    if name in ("Generator", "GeneratorTSM", "GeneratorRGB"):
        from . import model
        return getattr(model, name)
    if name == "ShadowSynth":
        from .shadow_synth_gpu import ShadowSynth
        return ShadowSynth
    if name == "TrainLosses":
        from .train_losses_gpu import TrainLosses
        return TrainLosses
    if name == "Discriminators":
        from .discriminator_gpu import Discriminators
        return Discriminators
    if name == "Perceptual":
        from .perceptual_gpu import Perceptual
        return Perceptual
    if name == "ColourTail":
        from .clr_tail_gpu import ColourTail
        return ColourTail
    if name == "ColourDecoder":
        from .clr_decoder_gpu import ColourDecoder
        return ColourDecoder
    if name == "NonLocalGrad":
        from .nonlocal_grad_gpu import NonLocalGrad
        return NonLocalGrad
    if name == "BottleneckGrad":
        from .bottleneck_grad_gpu import BottleneckGrad
        return BottleneckGrad
    if name == "HeadsGrad":
        from .heads_grad_gpu import HeadsGrad
        return HeadsGrad
    if name == "GreyDecoder":
        from .grey_decoder_gpu import GreyDecoder
        return GreyDecoder
    if name == "ColourTrunk":
        from .colour_trunk_gpu import ColourTrunk
        return ColourTrunk
    if name == "LowerTrunk":
        from .lower_trunk_gpu import LowerTrunk
        return LowerTrunk
    raise AttributeError(name)
