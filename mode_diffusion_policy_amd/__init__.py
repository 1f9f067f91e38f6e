"""MI355X-native MoDE denoising hot path (drop-in for the reference's MoDeDiT / GCDenoiser / sample_ddim)."""
from .modedit import MoDeDiT, NoiseBlockMoE  # noqa: F401
from .score_wrappers import GCDenoiser  # noqa: F401
from .gc_sampling import get_sigmas_exponential, sample_ddim  # noqa: F401
from .training import diffusion_loss, training_step  # noqa: F401
from .lang_buffer import AdvancedLangEmbeddingBuffer  # noqa: F401
from .perceptual_encoders import (FiLMResNet18Policy, FiLMResNet34Policy, FiLMResNet50Policy, GraphedVisualEncoder, ResNetEncoderWithFiLM,  # noqa: F401
                                  embed_visual_obs)
from .lora import LoraAdapter  # noqa: F401
from .camera import CLIP_MEAN, CLIP_STD, CameraTransform, preprocess_cameras  # noqa: F401
from . import data  # noqa: F401
from .data import EpisodeStore, WindowStream, WindowSweep, mixture_weights, split_episodes  # noqa: F401
from . import validation  # noqa: F401
from .validation import LevelResult, LevelValidator, Validator  # noqa: F401

__all__ = ["MoDeDiT", "NoiseBlockMoE", "GCDenoiser", "sample_ddim", "get_sigmas_exponential", "diffusion_loss", "training_step", "AdvancedLangEmbeddingBuffer",
           "FiLMResNet18Policy", "FiLMResNet34Policy", "FiLMResNet50Policy", "ResNetEncoderWithFiLM", "embed_visual_obs",
           "CameraTransform", "preprocess_cameras", "CLIP_MEAN", "CLIP_STD", "LoraAdapter", "data", "EpisodeStore", "WindowStream", "WindowSweep",
           "split_episodes", "mixture_weights", "validation", "Validator", "LevelValidator", "LevelResult"]
