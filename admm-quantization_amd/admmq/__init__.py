"""admmq — MI355X-native ADMM quantized CP/low-rank factorization.

Drop-in replacements for KamikaziZen/admm-quantization's hot path:

    source.admm.admm_iteration / init_factors / squared_relative_diff -> admmq.admm
    source.quantization.quantize_tensor (+ _mse, min_max_quantize)     -> admmq.quantization
      (packed integer codes + scale / zero-point of the tensor schemes) -> admmq.packed
    source.utils.unfold                                                 -> admmq.utils
    source.parafac_epc.parafac_epc                                      -> admmq.parafac_epc
    scripts/factorize.py (ALS driver + CLI)                             -> admmq.factorize
      (Gram∘Gram / MTTKRP / reconstruction error on the device)         -> admmq.als
    scripts/factorize_lowrank.py (quant + low-rank ADMM + CLI)          -> admmq.lowrank
    source.models.build_cp_layer / build_cp2conv_layer / ... (export)   -> admmq.export

Compute runs in libadmmq.so (hand-written HIP for gfx950) through a C ABI
(include/admmq.h); there is no CPU fallback.
"""
from .admm import admm_iteration, admm_iteration_batched, init_factors, init_factors_many, squared_relative_diff  # noqa: F401
from .quantization import quantize_tensor, quantize_tensor_mse, min_max_quantize, fixed_quantize, quantize_batched  # noqa: F401
from .packed import PackedTensor, quantize_packed, dequantize_packed, save_packed, load_packed  # noqa: F401
from .packed import packed_linear, packed_conv1x1, packed_depthwise_conv1x1  # noqa: F401
from .packed import QuantizedActivation, act_encode, act_decode, packed_rowsums  # noqa: F401
from .packed import packed_linear_int, packed_conv1x1_int  # noqa: F401
from .packed import packed_taps_int, packed_depthwise_conv1x1_int  # noqa: F401
from .packed import PackedLowRank, packed_lowrank_linear, save_packed_lowrank, load_packed_lowrank  # noqa: F401
from .utils import unfold  # noqa: F401

__version__ = "0.1.0"
