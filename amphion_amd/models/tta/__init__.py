"""AudioLDM text-to-audio inference on the HIP kernels (models/tta)."""
