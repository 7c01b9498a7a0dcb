"""runbooks_amd.ops — MI355X (gfx950) compute ops.

GPU tensors run on hand-written CDNA4 HIP kernels (csrc/); CPU tensors run
plain-PyTorch fp32 references (the numerics oracles). A GPU tensor with no
built extension raises — there is no silent eager fallback on the GPU.
"""
from ._backend import ext, has_hip, use_hip  # noqa: F401
from .activations import cross_entropy, swiglu  # noqa: F401
from .adamw import FusedAdamW  # noqa: F401
from .attention import (causal_attention, flash_prefill, paged_decode,  # noqa: F401
                        paged_decode_ref, paged_decode_with_operand,
                        paged_prefill, paged_prefill_batch,
                        paged_prefill_batch_ref, paged_prefill_plan,
                        paged_prefill_ref, paged_verify, paged_verify_ref)
from .kvcache import BLOCK_SIZE, alloc_kv_cache, kv_append, kv_append_ref  # noqa: F401
from .linear import (Linear, decode_layout, decode_linear_glu,  # noqa: F401
                     decode_linear_raw, decode_linear_rope_append,
                     fast_linear, fused_epilogue_ok, w4_prefill_enabled)
from .lora_serve import (lora_expand_, lora_expand_ref_, lora_shrink,  # noqa: F401
                         lora_shrink_ref)
from .norm import RMSNorm, rmsnorm, rmsnorm_ref  # noqa: F401
from .rope import rope, rope_ref, rope_tables  # noqa: F401
from .sampling import (SampleBatchResult, pack_sample_batch,  # noqa: F401
                       sample_batch, sample_batch_ref, sample_tokens)
