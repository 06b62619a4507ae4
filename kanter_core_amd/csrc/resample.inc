// What the separable resamplers of resize_tile.hip and resize_down.hip share.  Included inside namespace kc.
// ------------------------------------------------------------------------------------------
// Separable resample = image::imageops::resize (crate image 0.24.0) as called from
// src/shared.rs:159-199.  Weights come from host-built tap tables (resize.cpp) so they are the
// same f32 values the scalar algorithm computes; the sums run sequentially from 0.0, unfused.
// ------------------------------------------------------------------------------------------
static __device__ __forceinline__ float clamp01_nan_passthrough(float t)
{
    // image::math::utils::clamp: NaN compares false both ways and passes through.
    if (t < 0.0f) return 0.0f;
    if (t > 1.0f) return 1.0f;
    return t;
}
