from .adapter_models import ClipAdapterModel  # noqa: F401
from .cache_models import TipAdapterModel, group_keys_by_class  # noqa: F401
from .clip_encoders import CustomImageEncoder, CustomTextEncoder, ImageEncoder, TextEncoder  # noqa: F401
from .gda_models import GdaHeadModel  # noqa: F401
from .probe_models import LinearProbeModel  # noqa: F401
from .prompts_models import ImagePrefixModel, MaPLeModel, TextPrefixModel, UPTModel  # noqa: F401
