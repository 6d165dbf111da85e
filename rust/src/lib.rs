//! Rust shim: the public model API of Gadersd/stable-diffusion-xl-burn on top of `libsdxl_mi355.so`.
//!
//! The reference's types keep their names and signatures (file:line = the reference repository):
//!
//! | here                                         | replaces                                             |
//! |----------------------------------------------|------------------------------------------------------|
//! | `Conditioning<B>`                            | `src/model/stablediffusion/mod.rs:544-555`           |
//! | `Diffuser::<B>::sample_latent`               | `:317-332`                                           |
//! | `Diffuser::<B>::sample_latent_with_inpainting` | `:334-353`                                         |
//! | `Diffuser::<B>::refine_latent`               | `:355-376`                                           |
//! | `LatentDecoder::<B>::{latent_to_image, image_to_latent, encode_image, decode_latent}` | `:200-266`  |
//! | `Embedder::<B>::text_to_conditioning`        | `:661-696`                                           |
//! | `UNet::<B>::forward`                         | `src/model/unet/mod.rs:450-456`                      |
//! | `trait Backend { qkv_attention, attn_decoder_mask }` + `Mi355Attention` | `src/backend.rs:3-24`     |
//!
//! The reference draws its noise from an unseeded generator inside `sample_latent` (`gen_noise`, `:378-388`); the engine
//! takes noise as an argument so results are reproducible.  The reference-shaped methods therefore draw
//! `Tensor::random(Normal(0,1))` exactly where the reference does and forward to `*_with_noise` companions, which are the
//! ones parity tests use.  `Diffuser::set_seed` switches them to the `*_seeded` companions: every noise tensor is then drawn
//! on the device from one 64-bit seed per batch entry (`sdxl_gen_noise`, `sdxl_*_seeded`), the same bits as from C or Python.
//!
//! Tensors cross the boundary as fp32 device buffers in the reference's own layouts.  `bridge` is the generic path for ANY
//! burn backend (host hop, like the reference's own `DefaultBackendConverter`, `src/backend_converter.rs:25-39`); the
//! `tch-bridge` feature passes `data_ptr()` of burn-tch tensors that already live in HIP memory.
//!
//! Status: written against `include/sdxl_mi355.h`; NOT compiled in the build container (no cargo/rustc there).
#![allow(non_camel_case_types, non_upper_case_globals, non_snake_case, dead_code)]

pub mod ffi {
    include!(concat!(env!("OUT_DIR"), "/bindings.rs"));
}

use burn::tensor::{backend::Backend as BurnBackend, Bool, Data, Distribution, ElementConversion, Int, Shape, Tensor};
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;

// ------------------------------------------------------------------------------------------------ errors
/// model code in the reference asserts / unwraps (`unet/mod.rs:73-76`, `:967-972`, `groupnorm/mod.rs:19-24`): a non-zero
/// status from the engine becomes a panic carrying the engine's message, loaders get a `Result`
fn last_error() -> String {
    unsafe { CStr::from_ptr(ffi::sdxl_last_error()).to_string_lossy().into_owned() }
}
fn check(rc: c_int) {
    if rc != 0 {
        panic!("sdxl_mi355: {}", last_error());
    }
}
fn try_check(rc: c_int) -> Result<(), Box<dyn std::error::Error>> {
    if rc != 0 {
        Err(last_error().into())
    } else {
        Ok(())
    }
}

// ------------------------------------------------------------------------------------------------ HIP runtime (bridge)
extern "C" {
    fn hipMalloc(ptr: *mut *mut c_void, bytes: usize) -> c_int;
    fn hipFree(ptr: *mut c_void) -> c_int;
    fn hipMemcpy(dst: *mut c_void, src: *const c_void, bytes: usize, kind: c_int) -> c_int;
}
const HIP_MEMCPY_HOST_TO_DEVICE: c_int = 1;
const HIP_MEMCPY_DEVICE_TO_HOST: c_int = 2;

/// an owned fp32 (or raw byte) device buffer
pub struct DeviceBuf {
    ptr: *mut c_void,
    bytes: usize,
}
impl DeviceBuf {
    pub fn new(bytes: usize) -> Self {
        let mut p = ptr::null_mut();
        assert_eq!(unsafe { hipMalloc(&mut p, bytes.max(16)) }, 0, "hipMalloc({bytes}) failed");
        DeviceBuf { ptr: p, bytes }
    }
    pub fn from_f32(v: &[f32]) -> Self {
        let b = Self::new(v.len() * 4);
        assert_eq!(unsafe { hipMemcpy(b.ptr, v.as_ptr() as *const c_void, v.len() * 4, HIP_MEMCPY_HOST_TO_DEVICE) }, 0);
        b
    }
    pub fn from_u8(v: &[u8]) -> Self {
        let b = Self::new(v.len());
        assert_eq!(unsafe { hipMemcpy(b.ptr, v.as_ptr() as *const c_void, v.len(), HIP_MEMCPY_HOST_TO_DEVICE) }, 0);
        b
    }
    pub fn to_f32(&self) -> Vec<f32> {
        let mut v = vec![0f32; self.bytes / 4];
        assert_eq!(unsafe { hipMemcpy(v.as_mut_ptr() as *mut c_void, self.ptr, self.bytes, HIP_MEMCPY_DEVICE_TO_HOST) }, 0);
        v
    }
    pub fn to_u8(&self) -> Vec<u8> {
        let mut v = vec![0u8; self.bytes];
        assert_eq!(unsafe { hipMemcpy(v.as_mut_ptr() as *mut c_void, self.ptr, self.bytes, HIP_MEMCPY_DEVICE_TO_HOST) }, 0);
        v
    }
    pub fn f32_ptr(&self) -> *const f32 {
        self.ptr as *const f32
    }
    pub fn f32_mut(&self) -> *mut f32 {
        self.ptr as *mut f32
    }
}
impl Drop for DeviceBuf {
    fn drop(&mut self) {
        unsafe { hipFree(self.ptr) };
    }
}

/// burn tensor <-> fp32 device buffer, for any backend (host hop; see the module docs for the zero-copy feature)
pub mod bridge {
    use super::*;
    pub fn upload<B: BurnBackend, const D: usize>(t: Tensor<B, D>) -> DeviceBuf {
        let data: Data<f32, D> = t.into_data().convert();
        DeviceBuf::from_f32(&data.value)
    }
    pub fn upload_int<B: BurnBackend, const D: usize>(t: Tensor<B, D, Int>) -> (DeviceBuf, Vec<i32>) {
        let v: Vec<i32> = t.into_data().value.iter().map(|x| x.elem::<i32>()).collect();
        let b = DeviceBuf::new(v.len() * 4);
        assert_eq!(unsafe { hipMemcpy(b.ptr, v.as_ptr() as *const c_void, v.len() * 4, HIP_MEMCPY_HOST_TO_DEVICE) }, 0);
        (b, v)
    }
    pub fn download<B: BurnBackend, const D: usize>(b: &DeviceBuf, shape: [usize; D], device: &B::Device) -> Tensor<B, D> {
        Tensor::from_data(Data::new(b.to_f32(), Shape::new(shape)).convert(), device)
    }
}

// ------------------------------------------------------------------------------------------------ context / precision
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum Precision {
    /// strict parity with the fp32 CPU reference (exact-fp32 MFMA)
    F32 = ffi::SDXL_DTYPE_F32 as isize,
    /// fp16 storage and MFMA operands, fp32 accumulation (what `LibTorch<f16>` is in `src/bin/sample/main.rs:122`)
    F16 = ffi::SDXL_DTYPE_F16 as isize,
    F16F32Res = ffi::SDXL_DTYPE_F16_F32RES as isize,
    /// fp32-class results on the f16 matrix pipe: (hi, lo) f16 operand pairs, three MFMAs per product (UNet / Diffuser / VAE)
    F32Split = ffi::SDXL_DTYPE_F32_SPLIT as isize,
    /// `F32Split` with the self-attention and the GEGLU projection on plain f16 operands (UNet / Diffuser only): the fastest mode whose
    /// config-2 latents stay inside the parity tests' scaled 1e-3 bound
    F32SplitMix = ffi::SDXL_DTYPE_F32_SPLIT_MIX as isize,
    /// `F32SplitMix` for models whose parameters are f16 values (the `.mpk` records of `HalfPrecisionSettings`): QKV projection, both attentions'
    /// out-projections, FF-out and the cross-attention query projection on f16 operands as well, LayerNorms folded through an f16 shadow of the
    /// stream (`capi_internal.h` `mix_of`); on other parameters the engine falls back to `F32SplitMix`'s classes (`Diffuser::mix_classes`)
    F32SplitMixF16W = ffi::SDXL_DTYPE_F32_SPLIT_MIX_F16W as isize,
    /// `F32SplitMixF16W` with the GEGLU projection's activations as (hi, lo) f16 pairs along a doubled K (two MFMAs per product): ~12 % slower, inside the
    /// scaled bound on every fixture of the parity tests
    F32SplitMixF16WGeglu2 = ffi::SDXL_DTYPE_F32_SPLIT_MIX_F16W_GEGLU2 as isize,
    /// `F32Split` for models whose parameters are f16 values: the same fp32-class arithmetic with the transformer's linear layers on the f16 kernels (~10 % faster)
    F32SplitF16W = ffi::SDXL_DTYPE_F32_SPLIT_F16W as isize,
}

/// one per GPU (the reference hard-codes `LibTorchDevice::Cuda(0)`, `src/bin/sample/main.rs:131`)
pub struct Mi355Context {
    raw: *mut ffi::sdxl_ctx,
}
impl Mi355Context {
    pub fn new(device_id: i32) -> Result<Self, Box<dyn std::error::Error>> {
        let mut raw = ptr::null_mut();
        try_check(unsafe { ffi::sdxl_ctx_create(device_id, &mut raw) })?;
        Ok(Mi355Context { raw })
    }
    pub fn synchronize(&self) {
        check(unsafe { ffi::sdxl_ctx_synchronize(self.raw) });
    }
}
impl Drop for Mi355Context {
    fn drop(&mut self) {
        unsafe { ffi::sdxl_ctx_destroy(self.raw) };
    }
}

// ------------------------------------------------------------------------------------------------ Conditioning
/// `Conditioning<B>` of the reference, field for field (`stablediffusion/mod.rs:544-555`)
#[derive(Clone, Debug)]
pub struct Conditioning<B: BurnBackend> {
    pub unconditional_context_full: Tensor<B, 2>,
    pub unconditional_context_open_clip: Tensor<B, 2>,
    pub context_full: Tensor<B, 3>,
    pub context_open_clip: Tensor<B, 3>,
    pub unconditional_channel_context: Tensor<B, 1>,
    pub unconditional_channel_context_refiner: Tensor<B, 1>,
    pub channel_context: Tensor<B, 2>,
    pub channel_context_refiner: Tensor<B, 2>,
    pub resolution: [usize; 2], // (height, width)
}

/// the eight tensors on the device + the C view of them; the buffers live as long as this value
struct DeviceConditioning {
    _bufs: Vec<DeviceBuf>,
    c: ffi::sdxl_conditioning,
}
fn to_c_conditioning<B: BurnBackend>(c: &Conditioning<B>) -> DeviceConditioning {
    let [n, n_ctx, _] = c.context_full.dims();
    let bufs = vec![
        bridge::upload(c.unconditional_context_full.clone()),
        bridge::upload(c.unconditional_context_open_clip.clone()),
        bridge::upload(c.context_full.clone()),
        bridge::upload(c.context_open_clip.clone()),
        bridge::upload(c.unconditional_channel_context.clone()),
        bridge::upload(c.unconditional_channel_context_refiner.clone()),
        bridge::upload(c.channel_context.clone()),
        bridge::upload(c.channel_context_refiner.clone()),
    ];
    let raw = ffi::sdxl_conditioning {
        unconditional_context_full: bufs[0].f32_ptr(),
        unconditional_context_open_clip: bufs[1].f32_ptr(),
        context_full: bufs[2].f32_ptr(),
        context_open_clip: bufs[3].f32_ptr(),
        unconditional_channel_context: bufs[4].f32_ptr(),
        unconditional_channel_context_refiner: bufs[5].f32_ptr(),
        channel_context: bufs[6].f32_ptr(),
        channel_context_refiner: bufs[7].f32_ptr(),
        n: n as i32,
        n_ctx: n_ctx as i32,
        height: c.resolution[0] as i32,
        width: c.resolution[1] as i32,
    };
    DeviceConditioning { _bufs: bufs, c: raw }
}

// ------------------------------------------------------------------------------------------------ configs
/// `DiffuserConfig` (`stablediffusion/mod.rs:269-278`), same fields
#[derive(Clone, Debug)]
pub struct DiffuserConfig {
    pub adm_in_channels: usize,
    pub model_channels: usize,
    pub channel_mults: Vec<usize>,
    pub num_head_channels: usize,
    pub transformer_depths: Vec<usize>,
    pub context_dim: usize,
    pub is_refiner: bool,
}
impl DiffuserConfig {
    pub fn sdxl_base() -> Self {
        DiffuserConfig { adm_in_channels: 2816, model_channels: 320, channel_mults: vec![1, 2, 4], num_head_channels: 64,
                         transformer_depths: vec![0, 2, 10], context_dim: 2048, is_refiner: false }
    }
    pub fn sdxl_refiner() -> Self {
        DiffuserConfig { adm_in_channels: 2560, model_channels: 384, channel_mults: vec![1, 2, 4, 4], num_head_channels: 64,
                         transformer_depths: vec![0, 4, 4, 4], context_dim: 1280, is_refiner: true }
    }
    fn to_c(&self) -> ffi::sdxl_unet_config {
        assert!(self.channel_mults.len() == self.transformer_depths.len() && self.channel_mults.len() <= 8);
        let mut c: ffi::sdxl_unet_config = unsafe { std::mem::zeroed() };
        c.adm_in_channels = self.adm_in_channels as i32;
        c.in_channels = 4;
        c.out_channels = 4;
        c.model_channels = self.model_channels as i32;
        c.n_levels = self.channel_mults.len() as i32;
        for (i, (&m, &d)) in self.channel_mults.iter().zip(&self.transformer_depths).enumerate() {
            c.channel_mults[i] = m as i32;
            c.transformer_depths[i] = d as i32;
        }
        c.n_head_channels = self.num_head_channels as i32;
        c.context_dim = self.context_dim as i32;
        c.is_refiner = self.is_refiner as i32;
        c
    }
    /// replaces `DiffuserConfig::init` + `load_record` (`stablediffusion/mod.rs:281-305`, `bin/sample/main.rs:35-43`):
    /// `weights_flat` = the tensors of `sdxl_unet_param_spec` order back to back, fp32 (see `param_names`)
    pub fn init_with_weights<B: BurnBackend>(&self, ctx: &Mi355Context, precision: Precision, weights_flat: &[f32],
                                             alphas_cumprod: &[f32]) -> Result<Diffuser<B>, Box<dyn std::error::Error>> {
        let cfg = self.to_c();
        let need = param_numel(&cfg);
        if weights_flat.len() != need {
            return Err(format!("expected {need} weight values, got {}", weights_flat.len()).into());
        }
        let mut raw = ptr::null_mut();
        try_check(unsafe {
            ffi::sdxl_diffuser_create(ctx.raw, &cfg, precision as c_int, weights_flat.as_ptr(), alphas_cumprod.as_ptr(),
                                      alphas_cumprod.len() as c_int, &mut raw)
        })?;
        Ok(Diffuser { raw, n_steps: alphas_cumprod.len(), is_refiner: self.is_refiner, seed: std::cell::Cell::new(None), _b: std::marker::PhantomData })
    }
    /// seeded synthetic weights generated on the device (no checkpoint): what the parity tests and `bench.py` run
    pub fn init_synthetic<B: BurnBackend>(&self, ctx: &Mi355Context, precision: Precision, seed: u64, alphas_cumprod: &[f32]) -> Diffuser<B> {
        let cfg = self.to_c();
        let mut raw = ptr::null_mut();
        check(unsafe {
            ffi::sdxl_diffuser_create_synthetic(ctx.raw, &cfg, precision as c_int, seed, alphas_cumprod.as_ptr(),
                                                alphas_cumprod.len() as c_int, &mut raw)
        });
        Diffuser { raw, n_steps: alphas_cumprod.len(), is_refiner: self.is_refiner, seed: std::cell::Cell::new(None), _b: std::marker::PhantomData }
    }
    /// `init_with_weights` with create-time adapters merged into the UNet while it is built (`sdxl_diffuser_create_lora`): a static merged
    /// model, nothing changes per step.  `round_f16`: `SDXL_LORA_ROUND_F16`, adapted tensors rounded to f16 values (keeps the `*F16W` modes' classes)
    pub fn init_with_weights_lora<B: BurnBackend>(&self, ctx: &Mi355Context, precision: Precision, weights_flat: &[f32], adapters: &[LoraAdapter],
                                                  round_f16: bool, alphas_cumprod: &[f32]) -> Result<Diffuser<B>, Box<dyn std::error::Error>> {
        let cfg = self.to_c();
        let need = param_numel(&cfg);
        if weights_flat.len() != need {
            return Err(format!("expected {need} weight values, got {}", weights_flat.len()).into());
        }
        let entries = lora_entries(&cfg, adapters)?;
        let mut raw = ptr::null_mut();
        try_check(unsafe {
            ffi::sdxl_diffuser_create_lora(ctx.raw, &cfg, precision as c_int, weights_flat.as_ptr(), ptr::null(), 0, entries.as_ptr(),
                                           entries.len() as c_int, if round_f16 { ffi::SDXL_LORA_ROUND_F16 as c_int } else { 0 },
                                           alphas_cumprod.as_ptr(), alphas_cumprod.len() as c_int, &mut raw)
        })?;
        Ok(Diffuser { raw, n_steps: alphas_cumprod.len(), is_refiner: self.is_refiner, seed: std::cell::Cell::new(None), _b: std::marker::PhantomData })
    }
    /// `init_synthetic` with create-time adapters
    pub fn init_synthetic_lora<B: BurnBackend>(&self, ctx: &Mi355Context, precision: Precision, seed: u64, adapters: &[LoraAdapter], round_f16: bool,
                                               alphas_cumprod: &[f32]) -> Result<Diffuser<B>, Box<dyn std::error::Error>> {
        let cfg = self.to_c();
        let entries = lora_entries(&cfg, adapters)?;
        let mut raw = ptr::null_mut();
        try_check(unsafe {
            ffi::sdxl_diffuser_create_lora(ctx.raw, &cfg, precision as c_int, ptr::null(), ptr::null(), seed, entries.as_ptr(),
                                           entries.len() as c_int, if round_f16 { ffi::SDXL_LORA_ROUND_F16 as c_int } else { 0 },
                                           alphas_cumprod.as_ptr(), alphas_cumprod.len() as c_int, &mut raw)
        })?;
        Ok(Diffuser { raw, n_steps: alphas_cumprod.len(), is_refiner: self.is_refiner, seed: std::cell::Cell::new(None), _b: std::marker::PhantomData })
    }
}
/// One adapter on one parameter, already in the engine's layout (`sdxl_lora_entry`): `W += scale * left @ right` on the matrix view of parameter
/// `param_index` (`param_names` order), rows = shape[0], cols = the product of the other dimensions, `left` [rows, rank], `right` [rank, cols], row-major.
/// From the usual adapter tensors (`down.weight` [r, in...], `up.weight` [out, r]): a Linear parameter [d_in, d_out] takes `left = down^T`,
/// `right = up^T`; a Conv2d parameter [out, in, kh, kw] takes `left = up`, `right = down` flattened to [r, in * kh * kw].  `scale = strength * alpha / rank`.
#[derive(Clone, Debug)]
pub struct LoraAdapter {
    pub param_index: usize,
    pub rank: usize,
    pub left: Vec<f32>,
    pub right: Vec<f32>,
    pub scale: f32,
}
/// the C entries over host arrays the adapters own; extents are checked here (the C ABI cannot see them), the rest by `sdxl_lora_check`
fn lora_entries(cfg: &ffi::sdxl_unet_config, adapters: &[LoraAdapter]) -> Result<Vec<ffi::sdxl_lora_entry>, Box<dyn std::error::Error>> {
    let mut entries = Vec::with_capacity(adapters.len());
    for (i, a) in adapters.iter().enumerate() {
        let (mut name, mut ndim, mut shape, mut kind, mut sc, mut mean) = (ptr::null(), 0, [0i64; 4], 0, 0f32, 0f32);
        try_check(unsafe { ffi::sdxl_unet_param_spec(cfg, a.param_index as c_int, &mut name, &mut ndim, shape.as_mut_ptr(), &mut kind, &mut sc, &mut mean) })?;
        let rows = shape[0] as usize;
        let cols = shape[1..ndim as usize].iter().product::<i64>() as usize;
        if a.left.len() != rows * a.rank || a.right.len() != a.rank * cols {
            return Err(format!("lora adapter {i}: expected left {rows} x {} and right {} x {cols}", a.rank, a.rank).into());
        }
        entries.push(ffi::sdxl_lora_entry { param_index: a.param_index as i32, rank: a.rank as i32, left: a.left.as_ptr(), right: a.right.as_ptr(), scale: a.scale });
    }
    try_check(unsafe { ffi::sdxl_lora_check(cfg, entries.as_ptr(), entries.len() as c_int) })?;
    Ok(entries)
}
fn param_numel(cfg: &ffi::sdxl_unet_config) -> usize {
    let n = unsafe { ffi::sdxl_unet_param_count(cfg) };
    assert!(n > 0, "sdxl_mi355: {}", last_error());
    let mut total = 0usize;
    for i in 0..n {
        let (mut name, mut ndim, mut shape, mut kind, mut sc, mut mean) = (ptr::null(), 0, [0i64; 4], 0, 0f32, 0f32);
        check(unsafe { ffi::sdxl_unet_param_spec(cfg, i, &mut name, &mut ndim, shape.as_mut_ptr(), &mut kind, &mut sc, &mut mean) });
        total += shape[..ndim as usize].iter().product::<i64>() as usize;
    }
    total
}
/// the reference's struct-field paths of every parameter, in hand-over order (`unet/load.rs:286-401`)
pub fn param_names(cfg: &DiffuserConfig) -> Vec<(String, Vec<usize>)> {
    let c = cfg.to_c();
    let n = unsafe { ffi::sdxl_unet_param_count(&c) };
    (0..n)
        .map(|i| {
            let (mut name, mut ndim, mut shape, mut kind, mut sc, mut mean) = (ptr::null(), 0, [0i64; 4], 0, 0f32, 0f32);
            check(unsafe { ffi::sdxl_unet_param_spec(&c, i, &mut name, &mut ndim, shape.as_mut_ptr(), &mut kind, &mut sc, &mut mean) });
            (unsafe { CStr::from_ptr(name) }.to_string_lossy().into_owned(), shape[..ndim as usize].iter().map(|&d| d as usize).collect())
        })
        .collect()
}

// ------------------------------------------------------------------------------------------------ Diffuser
/// `Diffuser<B>` (`stablediffusion/mod.rs:308-542`): the DDIM loop, CFG pair and UNet run on the MI355X
pub struct Diffuser<B: BurnBackend> {
    raw: *mut ffi::sdxl_diffuser,
    n_steps: usize,
    is_refiner: bool,
    /// `set_seed`: (seed of batch entry 0, eta) for the reference-shaped methods; `None` = unseeded `Tensor::random`
    seed: std::cell::Cell<Option<(u64, f64)>>,
    _b: std::marker::PhantomData<B>,
}
/// draw numbers of the seeded noise (`SDXL_DRAW_*` of the header; bindgen does not translate function-like macros)
pub const DRAW_INITIAL: u32 = 0;
pub const fn draw_blend(i: u32) -> u32 {
    1 + 2 * i
}
pub const fn draw_sigma(i: u32) -> u32 {
    2 + 2 * i
}
/// the update behind every UNet evaluation (`SDXL_SOLVER_*`): a per-handle option all trajectory methods honour
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Solver {
    /// the reference's DDIM loop (`:390-432`), the default
    Ddim = ffi::SDXL_SOLVER_DDIM as isize,
    /// DPM-Solver++(2M) on the same schedule, with `eta > 0` its SDE form: second order at one UNet evaluation per iteration
    Dpmpp2M = ffi::SDXL_SOLVER_DPMPP_2M as isize,
    /// LCM multistep consistency sampling (Luo et al. 2023): jumps to the data prediction and re-noises it with fresh noise every iteration.
    /// Takes no `eta` (it must be 0) and needs a seed (`set_seed`) beyond a one-entry list
    Lcm = ffi::SDXL_SOLVER_LCM as isize,
    /// TCD gamma-sampling (Zheng et al. 2024; what Hyper-SD ships with): `eta` of `set_seed` is read as gamma
    Tcd = ffi::SDXL_SOLVER_TCD as isize,
    /// DPM++ 3M SDE (k-diffusion's `sample_dpmpp_3m_sde`; `eta = 0` its ODE form): the 2M update with a second history term, the usual
    /// companion of the Karras and exponential sigma spacings at 20-40 steps
    Dpmpp3M = ffi::SDXL_SOLVER_DPMPP_3M as isize,
}
/// a published sigma spacing (`SDXL_SIGMAS_*`) for `sigma_schedule`
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum SigmaSchedule {
    /// Karras et al. 2022, eq. 5 with exponent `rho` (7)
    Karras = ffi::SDXL_SIGMAS_KARRAS as isize,
    /// log-linear between sigma_max and sigma_min
    Exponential = ffi::SDXL_SIGMAS_EXPONENTIAL as isize,
    /// the sigmas of the reference rule's timestep list
    OfTimesteps = ffi::SDXL_SIGMAS_OF_TIMESTEPS as isize,
}
/// `sdxl_sigma_schedule` (host logic, no device): the list of `kind` for `Diffuser::set_sigmas`; `sigma_min` / `sigma_max` <= 0 take the ends of
/// the `alphas_cumprod` table.  What the engine refuses is an `Err` with its message.
pub fn sigma_schedule(kind: SigmaSchedule, n_steps: usize, alphas_cumprod: &[f32], sigma_min: f64, sigma_max: f64, rho: f64)
                      -> Result<Vec<f64>, Box<dyn std::error::Error>> {
    let mut out = vec![-1f64; alphas_cumprod.len().max(1)];      // a refusal leaves `out` untouched: SDXL_ERR_INVALID (1) is also a valid count
    let n = unsafe {
        ffi::sdxl_sigma_schedule(kind as c_int, n_steps as c_int, alphas_cumprod.as_ptr(), alphas_cumprod.len() as c_int, sigma_min, sigma_max, rho,
                                 out.as_mut_ptr(), out.len() as c_int)
    };
    if n < 1 || out[0] < 0.0 {
        return Err(last_error().into());
    }
    out.truncate(n as usize);
    Ok(out)
}
/// a published timestep spacing (`SDXL_SCHEDULE_*`) for `timestep_schedule`
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Schedule {
    /// the reference's rule as a list: `sdxl_step_count` entries
    Reference = ffi::SDXL_SCHEDULE_REFERENCE as isize,
    /// diffusers' "trailing" spacing (Lightning, Turbo)
    Trailing = ffi::SDXL_SCHEDULE_TRAILING as isize,
    /// diffusers' "leading" spacing; `param` is `steps_offset` (1 for SDXL)
    Leading = ffi::SDXL_SCHEDULE_LEADING as isize,
    /// the LCM / TCD / Hyper-SD schedule; `param` is the number of origin steps (50 for the published checkpoints)
    Lcm = ffi::SDXL_SCHEDULE_LCM as isize,
}
/// `sdxl_timestep_schedule` (host logic, no device): the list of `kind` for `Diffuser::set_timesteps`.  What the engine refuses is an `Err`
/// with its message.
pub fn timestep_schedule(kind: Schedule, n_steps: usize, n_train_steps: usize, param: i32) -> Result<Vec<i32>, Box<dyn std::error::Error>> {
    let mut out = vec![-1i32; n_train_steps.max(1)];      // a refusal leaves `out` untouched: SDXL_ERR_INVALID (1) is also a valid count
    let n = unsafe { ffi::sdxl_timestep_schedule(kind as c_int, n_steps as c_int, n_train_steps as c_int, param as c_int, out.as_mut_ptr(), out.len() as c_int) };
    if n < 1 || out[0] < 0 {
        return Err(last_error().into());
    }
    out.truncate(n as usize);
    Ok(out)
}
/// what the UNet's output means (`SDXL_PREDICTION_*`): a per-handle option all trajectory methods honour
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Prediction {
    /// the noise `e`, the reference's reading and the default
    Epsilon = ffi::SDXL_PREDICTION_EPSILON as isize,
    /// `v = alpha e - sigma x0`: checkpoints trained on a zero-terminal-SNR schedule (Lin et al. 2023); admits `alphas_cumprod == 0` at
    /// an iteration's own timestep
    V = ffi::SDXL_PREDICTION_V as isize,
}
/// `sdxl_rescale_zero_terminal_snr` (host logic, no device): the `alphas_cumprod` table shifted and scaled in sqrt-space so that its last
/// value is exactly 0 and its first unchanged (Lin et al. 2023, Algorithm 1).  A table with fewer than two values, a value outside (0, 1)
/// or one that is not strictly decreasing is an `Err` with the engine's message.
pub fn rescale_zero_terminal_snr(alphas_cumprod: &[f32]) -> Result<Vec<f32>, Box<dyn std::error::Error>> {
    let mut out = vec![0f32; alphas_cumprod.len()];
    try_check(unsafe { ffi::sdxl_rescale_zero_terminal_snr(alphas_cumprod.as_ptr(), alphas_cumprod.len() as c_int, out.as_mut_ptr()) })?;
    Ok(out)
}
/// how the two UNet branches of an iteration become the noise prediction (`sdxl_guidance`): a per-handle option all trajectory methods
/// honour.  `Guidance::default()` is the reference's line, one scalar scale on every iteration.
#[derive(Clone, Debug, PartialEq)]
pub struct Guidance {
    /// `SDXL_GUIDANCE_OFF`: the conditional branch alone as a batch-n forward (distilled checkpoints); takes no other option
    pub off: bool,
    /// phi of CFG rescale (Lin et al. 2023, section 3.4) in [0, 1]; 0.0 = off
    pub rescale: f32,
    /// one guidance scale per batch entry (at most 8), replacing the call's scalar; empty = the call's scalar
    pub scales: Vec<f32>,
    /// guidance only on iterations whose timestep `t` has `t_lo <= t <= t_hi`; `None` = every iteration
    pub t_range: Option<(i32, i32)>,
}
impl Default for Guidance {
    fn default() -> Self {
        Guidance { off: false, rescale: 0.0, scales: Vec::new(), t_range: None }
    }
}
impl Guidance {
    fn to_c(&self) -> ffi::sdxl_guidance {
        let mut g: ffi::sdxl_guidance = unsafe { std::mem::zeroed() };
        unsafe { ffi::sdxl_guidance_default(&mut g) };
        g.mode = if self.off { ffi::SDXL_GUIDANCE_OFF as i32 } else { ffi::SDXL_GUIDANCE_CFG as i32 };
        g.rescale = self.rescale;
        g.n_scales = self.scales.len() as i32;      // more than 8: the engine reports it
        for (dst, src) in g.scales.iter_mut().zip(self.scales.iter()) {
            *dst = *src;
        }
        if let Some((lo, hi)) = self.t_range {
            g.t_lo = lo;
            g.t_hi = hi;
        }
        g
    }
}
/// `SDXL_MAX_CONTROLS`: sources of one `sdxl_skip_residual_add_steps_multi` launch
pub const MAX_CONTROLS: usize = ffi::SDXL_MAX_CONTROLS as usize;
/// how a control net's residuals enter a trajectory, as a scale per iteration and batch entry (`sdxl_control`).  `Control::default()` is scale 1
/// for every entry on every iteration.  `Control::scale_table` is the table they describe; the `Diffuser` does not take a control net yet.
#[derive(Clone, Debug, PartialEq)]
pub struct Control {
    /// the conditioning scale of every entry
    pub scale: f32,
    /// one scale per batch entry (at most 8), replacing `scale`; empty = `scale`
    pub scales: Vec<f32>,
    /// control only on iterations whose timestep `t` has `t_lo <= t <= t_hi` (diffusers' `control_guidance_start / _end`); `None` = every iteration
    pub t_range: Option<(i32, i32)>,
    /// residuals for the conditional entries of the CFG pair only
    pub cond_only: bool,
}
impl Default for Control {
    fn default() -> Self {
        Control { scale: 1.0, scales: Vec::new(), t_range: None, cond_only: false }
    }
}
impl Control {
    fn to_c(&self) -> ffi::sdxl_control {
        let mut c: ffi::sdxl_control = unsafe { std::mem::zeroed() };
        unsafe { ffi::sdxl_control_default(&mut c) };
        c.scale = self.scale;
        c.n_scales = self.scales.len() as i32;      // more than 8: the engine reports it
        for (dst, src) in c.scales.iter_mut().zip(self.scales.iter()) {
            *dst = *src;
        }
        if let Some((lo, hi)) = self.t_range {
            c.t_lo = lo;
            c.t_hi = hi;
        }
        c.cond_only = self.cond_only as i32;
        c
    }
    /// `sdxl_control_scale_table` (host logic only): the scales of one control net over a trajectory, `timesteps.len() + 1` rows of 8 -- row `i` for the
    /// iteration at `timesteps[i]`, column `b` for batch entry `b` (`n` entries with `single_branch`, else the `2 n` of the CFG pair), the last row zeros
    pub fn scale_table(&self, n: usize, single_branch: bool, timesteps: &[i32]) -> Result<Vec<[f32; 8]>, Box<dyn std::error::Error>> {
        let c = self.to_c();
        let mut out = vec![[0f32; 8]; timesteps.len() + 1];
        try_check(unsafe {
            ffi::sdxl_control_scale_table(&c, n as c_int, single_branch as c_int, timesteps.as_ptr(), timesteps.len() as c_int, out.as_mut_ptr() as *mut f32)
        })?;
        Ok(out)
    }
    /// `sdxl_control_check` (host logic only): what the engine refuses about these options, for one branch or the CFG pair
    pub fn check(&self, single_branch: bool) -> Result<(), Box<dyn std::error::Error>> {
        let c = self.to_c();
        try_check(unsafe { ffi::sdxl_control_check(&c, single_branch as c_int) })
    }
}
impl<B: BurnBackend> Drop for Diffuser<B> {
    fn drop(&mut self) {
        unsafe { ffi::sdxl_diffuser_destroy(self.raw) };
    }
}
/// A ControlNet (`sdxl_controlnet`) for the UNet a `DiffuserConfig` describes: that UNet's encoder, a hint embedder and one 1x1 convolution per
/// skip tensor.  `Precision::F32`, `F16` or `F32Split`.
pub struct ControlNet {
    raw: *mut ffi::sdxl_controlnet,
}
impl Drop for ControlNet {
    fn drop(&mut self) {
        unsafe { ffi::sdxl_controlnet_destroy(self.raw) };
    }
}
impl ControlNet {
    fn config(cfg: &DiffuserConfig) -> ffi::sdxl_controlnet_config {
        let unet = cfg.to_c();
        let mut c: ffi::sdxl_controlnet_config = unsafe { std::mem::zeroed() };
        unsafe { ffi::sdxl_controlnet_config_default(&unet, &mut c) };
        c
    }
    /// number of f32 values `from_flat` expects (`sdxl_controlnet_param_spec` order)
    pub fn param_numel(cfg: &DiffuserConfig) -> usize {
        let c = Self::config(cfg);
        let n = unsafe { ffi::sdxl_controlnet_param_count(&c) };
        assert!(n >= 0, "sdxl_mi355: {}", last_error());
        let mut total = 0usize;
        for i in 0..n {
            let (mut ndim, mut shape): (c_int, [i64; 4]) = (0, [1; 4]);
            check(unsafe {
                ffi::sdxl_controlnet_param_spec(&c, i, ptr::null_mut(), &mut ndim, shape.as_mut_ptr(), ptr::null_mut(), ptr::null_mut(), ptr::null_mut())
            });
            total += shape.iter().take(ndim as usize).product::<i64>() as usize;
        }
        total
    }
    /// seeded synthetic weights (`sdxl_controlnet_create_synthetic`); a refiner configuration or another precision is an `Err`
    pub fn synthetic(ctx: &Mi355Context, cfg: &DiffuserConfig, precision: Precision, seed: u64) -> Result<Self, Box<dyn std::error::Error>> {
        let c = Self::config(cfg);
        let mut raw = ptr::null_mut();
        try_check(unsafe { ffi::sdxl_controlnet_create_synthetic(ctx.raw, &c, precision as c_int, seed, &mut raw) })?;
        Ok(ControlNet { raw })
    }
    /// the control forward (`sdxl_controlnet_forward`): hint `[B, 3, 8h, 8w]` for the latent `x` `[B, 4, h, w]` -> the residual tensors
    /// (`sdxl_unet_skip_shape` order: one per input entry, then the middle block's), what `Diffuser::unet_forward_residuals` takes
    pub fn forward<B: BurnBackend>(&self, cfg: &DiffuserConfig, x: Tensor<B, 4>, timesteps: Tensor<B, 1, Int>, context: Tensor<B, 3>, label: Tensor<B, 2>,
                                   hint: Tensor<B, 4>) -> Result<Vec<Tensor<B, 4>>, Box<dyn std::error::Error>> {
        let device = x.device();
        let [b, _, h, w] = x.dims();
        let [_, n_ctx, _] = context.dims();
        let uc = cfg.to_c();
        let count = unsafe { ffi::sdxl_unet_skip_count(&uc) };
        if count < 0 {
            return Err(last_error().into());
        }
        let mut shapes = Vec::new();
        for i in 0..count {
            let mut chw = [0i64; 3];
            try_check(unsafe { ffi::sdxl_unet_skip_shape(&uc, i, h as c_int, w as c_int, chw.as_mut_ptr()) })?;
            shapes.push([b, chw[0] as usize, chw[1] as usize, chw[2] as usize]);
        }
        let total: usize = shapes.iter().map(|s| s.iter().product::<usize>()).sum();
        let (d_x, (d_t, _), d_c, d_y, d_h) =
            (bridge::upload(x), bridge::upload_int(timesteps), bridge::upload(context), bridge::upload(label), bridge::upload(hint));
        let out = DeviceBuf::new(total * 4);
        try_check(unsafe {
            ffi::sdxl_controlnet_forward(self.raw, ptr::null_mut(), d_x.f32_ptr(), d_t.ptr as *const i32, d_c.f32_ptr(), d_y.f32_ptr(), d_h.f32_ptr(),
                                         b as c_int, h as c_int, w as c_int, n_ctx as c_int, out.f32_mut())
        })?;
        let host = out.to_f32();
        let mut res = Vec::new();
        let mut o = 0usize;
        for s in shapes {
            let n: usize = s.iter().product();
            res.push(Tensor::from_data(Data::new(host[o..o + n].to_vec(), Shape::new(s)).convert(), &device));
            o += n;
        }
        Ok(res)
    }
    /// flat f32 weights in `sdxl_controlnet_param_spec` order (`sdxl_controlnet_create`)
    pub fn from_flat(ctx: &Mi355Context, cfg: &DiffuserConfig, precision: Precision, weights: &[f32]) -> Result<Self, Box<dyn std::error::Error>> {
        if weights.len() != Self::param_numel(cfg) {
            return Err(format!("ControlNet::from_flat: {} values given, the configuration takes {}", weights.len(), Self::param_numel(cfg)).into());
        }
        let c = Self::config(cfg);
        let mut raw = ptr::null_mut();
        try_check(unsafe { ffi::sdxl_controlnet_create(ctx.raw, &c, precision as c_int, weights.as_ptr(), &mut raw) })?;
        Ok(ControlNet { raw })
    }
}
impl<B: BurnBackend> Diffuser<B> {
    /// reference signature (`:317-322`); noise = `gen_noise` (`:378-388`)
    pub fn sample_latent(&self, conditioning: Conditioning<B>, unconditional_guidance_scale: f64, n_steps: usize) -> Tensor<B, 4> {
        if let Some((seed, eta)) = self.seed.get() {
            let seeds = Self::entry_seeds(seed, &conditioning);
            return self.sample_latent_seeded(conditioning, unconditional_guidance_scale, n_steps, &seeds, eta);
        }
        let noise = Self::gen_noise(&conditioning);
        self.sample_latent_with_noise(conditioning, unconditional_guidance_scale, n_steps, noise)
    }
    pub fn sample_latent_with_noise(&self, conditioning: Conditioning<B>, unconditional_guidance_scale: f64, n_steps: usize,
                                    noise0: Tensor<B, 4>) -> Tensor<B, 4> {
        let device = conditioning.context_full.device();
        let dims = noise0.dims();
        let dc = to_c_conditioning(&conditioning);
        let noise = bridge::upload(noise0);
        let out = DeviceBuf::new(dims.iter().product::<usize>() * 4);
        check(unsafe {
            ffi::sdxl_sample_latent(self.raw, ptr::null_mut(), &dc.c, unconditional_guidance_scale, n_steps as c_int, noise.f32_ptr(), out.f32_mut())
        });
        bridge::download(&out, dims, &device)
    }
    /// reference signature (`:334-341`): mask true = keep the generated latent (`mask_where`, `:465`); the per-step re-noise
    /// of the reference (`:463`) is drawn here, one `gen_noise` per iteration
    pub fn sample_latent_with_inpainting(&self, conditioning: Conditioning<B>, unconditional_guidance_scale: f64, n_steps: usize,
                                         reference: Tensor<B, 4>, mask: Tensor<B, 4, Bool>) -> Tensor<B, 4> {
        if let Some((seed, eta)) = self.seed.get() {
            let seeds = Self::entry_seeds(seed, &conditioning);
            return self.sample_latent_with_inpainting_seeded(conditioning, unconditional_guidance_scale, n_steps, reference, mask, &seeds, eta);
        }
        let iters = unsafe { ffi::sdxl_step_count(n_steps as c_int, 0, self.n_steps as c_int) } as usize;
        let noise0 = Self::gen_noise(&conditioning);
        let step_noise: Vec<Tensor<B, 4>> = (0..iters).map(|_| Self::gen_noise(&conditioning)).collect();
        self.sample_latent_with_inpainting_and_noise(conditioning, unconditional_guidance_scale, n_steps, reference, mask, noise0, step_noise)
    }
    #[allow(clippy::too_many_arguments)]
    pub fn sample_latent_with_inpainting_and_noise(&self, conditioning: Conditioning<B>, unconditional_guidance_scale: f64, n_steps: usize,
                                                   reference: Tensor<B, 4>, mask: Tensor<B, 4, Bool>, noise0: Tensor<B, 4>,
                                                   step_noise: Vec<Tensor<B, 4>>) -> Tensor<B, 4> {
        let device = conditioning.context_full.device();
        let dims = noise0.dims();
        let dc = to_c_conditioning(&conditioning);
        let mask_u8: Vec<u8> = mask.into_data().value.iter().map(|&m| m as u8).collect();
        let (d_ref, d_mask, d_noise) = (bridge::upload(reference), DeviceBuf::from_u8(&mask_u8), bridge::upload(noise0));
        let d_steps = bridge::upload(Tensor::cat(step_noise.into_iter().map(|t| t.unsqueeze::<5>()).collect(), 0));
        let out = DeviceBuf::new(dims.iter().product::<usize>() * 4);
        check(unsafe {
            ffi::sdxl_sample_latent_with_inpainting(self.raw, ptr::null_mut(), &dc.c, unconditional_guidance_scale, n_steps as c_int,
                                                    d_ref.f32_ptr(), d_mask.ptr as *const u8, d_noise.f32_ptr(), d_steps.f32_ptr(), out.f32_mut())
        });
        bridge::download(&out, dims, &device)
    }
    /// reference signature (`:355-362`)
    pub fn refine_latent(&self, latent: Tensor<B, 4>, conditioning: Conditioning<B>, unconditional_guidance_scale: f64, step_start: usize,
                         n_steps: usize) -> Tensor<B, 4> {
        if let Some((seed, eta)) = self.seed.get() {
            let seeds = Self::entry_seeds(seed, &conditioning);
            return self.refine_latent_seeded(latent, conditioning, unconditional_guidance_scale, step_start, n_steps, &seeds, eta);
        }
        let noise = Self::gen_noise(&conditioning);
        self.refine_latent_with_noise(latent, conditioning, unconditional_guidance_scale, step_start, n_steps, noise)
    }
    pub fn refine_latent_with_noise(&self, latent: Tensor<B, 4>, conditioning: Conditioning<B>, unconditional_guidance_scale: f64,
                                    step_start: usize, n_steps: usize, noise: Tensor<B, 4>) -> Tensor<B, 4> {
        let device = conditioning.context_full.device();
        let dims = latent.dims();
        let dc = to_c_conditioning(&conditioning);
        let (d_lat, d_noise) = (bridge::upload(latent), bridge::upload(noise));
        let out = DeviceBuf::new(dims.iter().product::<usize>() * 4);
        check(unsafe {
            ffi::sdxl_refine_latent(self.raw, ptr::null_mut(), d_lat.f32_ptr(), &dc.c, unconditional_guidance_scale, step_start as c_int,
                                    n_steps as c_int, d_noise.f32_ptr(), out.f32_mut())
        });
        bridge::download(&out, dims, &device)
    }
    /// From now on the reference-shaped methods draw their noise on the device: batch entry `b` uses `seed + b` (wrapping),
    /// `eta` in [0, 1] scales the `gen_noise() * sigma` term of `:427` (0.0 = the reference's update).  `None` restores the
    /// unseeded `Tensor::random` path.
    pub fn set_seed(&self, seed: Option<u64>, eta: f64) {
        self.seed.set(seed.map(|s| (s, eta)));
    }
    /// every following trajectory of this handle runs `solver` (`sdxl_diffuser_set_solver`)
    pub fn set_solver(&self, solver: Solver) {
        check(unsafe { ffi::sdxl_diffuser_set_solver(self.raw, solver as c_int) });
    }
    pub fn solver(&self) -> Solver {
        let mut v: c_int = 0;
        check(unsafe { ffi::sdxl_diffuser_get_solver(self.raw, &mut v) });
        match v {
            x if x == Solver::Dpmpp2M as c_int => Solver::Dpmpp2M,
            x if x == Solver::Lcm as c_int => Solver::Lcm,
            x if x == Solver::Tcd as c_int => Solver::Tcd,
            x if x == Solver::Dpmpp3M as c_int => Solver::Dpmpp3M,
            _ => Solver::Ddim,
        }
    }
    /// every following trajectory of this handle runs one UNet evaluation per entry of `timesteps`, a strictly decreasing list of training
    /// timesteps, and its `n_steps` must equal the list's length (`sdxl_diffuser_set_timesteps`); `None` goes back to the reference's rule.
    /// A list the engine refuses is an `Err` with its message, and the handle keeps what it had.
    pub fn set_timesteps(&self, timesteps: Option<&[i32]>) -> Result<(), Box<dyn std::error::Error>> {
        let (p, n) = match timesteps {
            Some(t) if !t.is_empty() => (t.as_ptr(), t.len() as c_int),
            _ => (ptr::null(), 0),
        };
        try_check(unsafe { ffi::sdxl_diffuser_set_timesteps(self.raw, p, n) })
    }
    /// `set_timesteps` with an end level: the last iteration lands on `alphas[t_end]` instead of the data (`sdxl_diffuser_set_timesteps_end`;
    /// `t_end` below the last entry, -1: the complete trajectory).  The latent it returns is the one `continue_latent` of another handle takes.
    pub fn set_timesteps_end(&self, timesteps: &[i32], t_end: i32) -> Result<(), Box<dyn std::error::Error>> {
        try_check(unsafe { ffi::sdxl_diffuser_set_timesteps_end(self.raw, timesteps.as_ptr(), timesteps.len() as c_int, t_end as c_int) })
    }
    /// every following trajectory of this handle runs one UNet evaluation per entry of `sigmas`, a strictly decreasing list of noise levels
    /// sigma = sqrt((1 - a) / a) (`sigma_schedule`), and ends on `sigma_end` (0: the complete trajectory); `round_t` feeds the UNet integer
    /// timesteps (`SDXL_SIGMAS_ROUND_T`).  `None` drops the list: the handle is back on its timestep list or rule (`sdxl_diffuser_set_sigmas`).
    pub fn set_sigmas(&self, sigmas: Option<&[f64]>, sigma_end: f64, round_t: bool) -> Result<(), Box<dyn std::error::Error>> {
        let (p, n) = match sigmas {
            Some(s) if !s.is_empty() => (s.as_ptr(), s.len() as c_int),
            _ => (ptr::null(), 0),
        };
        try_check(unsafe { ffi::sdxl_diffuser_set_sigmas(self.raw, p, n, sigma_end, if round_t { ffi::SDXL_SIGMAS_ROUND_T as c_int } else { 0 }) })
    }
    /// the handle's sigma list with its end level, `None` without one (`sdxl_diffuser_get_sigmas`)
    pub fn sigmas(&self) -> Option<(Vec<f64>, f64)> {
        let mut out = vec![-1f64; 4096];
        let mut end = 0f64;
        let n = unsafe { ffi::sdxl_diffuser_get_sigmas(self.raw, out.as_mut_ptr(), out.len() as c_int, &mut end, ptr::null_mut()) };
        if n < 1 || out[0] < 0.0 {
            return None;
        }
        out.truncate(n as usize);
        Some((out, end))
    }
    /// the handle's list, `None` for the reference's rule (`sdxl_diffuser_get_timesteps`)
    pub fn timesteps(&self) -> Option<Vec<i32>> {
        let mut out = vec![-1i32; 4096];
        let n = unsafe { ffi::sdxl_diffuser_get_timesteps(self.raw, out.as_mut_ptr(), out.len() as c_int) };
        if n < 1 || out[0] < 0 {
            return None;
        }
        out.truncate(n as usize);
        Some(out)
    }
    /// every following trajectory of this handle reads the UNet's output as `prediction` (`sdxl_diffuser_set_prediction`)
    pub fn set_prediction(&self, prediction: Prediction) {
        check(unsafe { ffi::sdxl_diffuser_set_prediction(self.raw, prediction as c_int) });
    }
    pub fn prediction(&self) -> Prediction {
        let mut v: c_int = 0;
        check(unsafe { ffi::sdxl_diffuser_get_prediction(self.raw, &mut v) });
        if v == Prediction::V as c_int { Prediction::V } else { Prediction::Epsilon }
    }
    /// every following trajectory of this handle runs `guidance` (`sdxl_diffuser_set_guidance`); options the engine refuses
    /// (`sdxl_guidance_check`: values out of range, anything but the default or `off` on a refiner) are an `Err` with its message and
    /// leave the handle as it was
    pub fn set_guidance(&self, guidance: &Guidance) -> Result<(), Box<dyn std::error::Error>> {
        let g = guidance.to_c();
        try_check(unsafe { ffi::sdxl_diffuser_set_guidance(self.raw, &g) })
    }
    fn entry_seeds(seed: u64, conditioning: &Conditioning<B>) -> Vec<u64> {
        let [n, _, _] = conditioning.context_full.dims();
        (0..n as u64).map(|b| seed.wrapping_add(b)).collect()
    }
    /// `gen_noise` (`:378-388`) with one seed per batch entry: `[seeds.len(), 4, height / 8, width / 8]` (`sdxl_gen_noise`)
    pub fn gen_noise_seeded(ctx: &Mi355Context, seeds: &[u64], draw: u32, resolution: [usize; 2], device: &B::Device) -> Tensor<B, 4> {
        let dims = [seeds.len(), 4, resolution[0] / 8, resolution[1] / 8];
        let out = DeviceBuf::new(dims.iter().product::<usize>() * 4);
        check(unsafe {
            ffi::sdxl_gen_noise(ctx.raw, ptr::null_mut(), seeds.as_ptr(), draw, dims[0] as c_int, dims[2] as c_int, dims[3] as c_int, out.f32_mut())
        });
        bridge::download(&out, dims, device)
    }
    /// `sample_latent` with `gen_noise` played by the device generator (`sdxl_sample_latent_seeded`): one seed per batch entry
    pub fn sample_latent_seeded(&self, conditioning: Conditioning<B>, unconditional_guidance_scale: f64, n_steps: usize, seeds: &[u64],
                                eta: f64) -> Tensor<B, 4> {
        let device = conditioning.context_full.device();
        let [n, _, _] = conditioning.context_full.dims();
        assert_eq!(seeds.len(), n, "one seed per batch entry");
        let dims = [n, 4, conditioning.resolution[0] / 8, conditioning.resolution[1] / 8];
        let dc = to_c_conditioning(&conditioning);
        let out = DeviceBuf::new(dims.iter().product::<usize>() * 4);
        check(unsafe {
            ffi::sdxl_sample_latent_seeded(self.raw, ptr::null_mut(), &dc.c, unconditional_guidance_scale, n_steps as c_int, seeds.as_ptr(), eta,
                                           out.f32_mut())
        });
        bridge::download(&out, dims, &device)
    }
    /// inpainting without noise tensors: the blend noise of `:463` is drawn inside the per-step kernel
    #[allow(clippy::too_many_arguments)]
    pub fn sample_latent_with_inpainting_seeded(&self, conditioning: Conditioning<B>, unconditional_guidance_scale: f64, n_steps: usize,
                                                reference: Tensor<B, 4>, mask: Tensor<B, 4, Bool>, seeds: &[u64], eta: f64) -> Tensor<B, 4> {
        let device = conditioning.context_full.device();
        let dims = reference.dims();
        assert_eq!(seeds.len(), dims[0], "one seed per batch entry");
        let dc = to_c_conditioning(&conditioning);
        let mask_u8: Vec<u8> = mask.into_data().value.iter().map(|&m| m as u8).collect();
        let (d_ref, d_mask) = (bridge::upload(reference), DeviceBuf::from_u8(&mask_u8));
        let out = DeviceBuf::new(dims.iter().product::<usize>() * 4);
        check(unsafe {
            ffi::sdxl_sample_latent_with_inpainting_seeded(self.raw, ptr::null_mut(), &dc.c, unconditional_guidance_scale, n_steps as c_int,
                                                           d_ref.f32_ptr(), d_mask.ptr as *const u8, seeds.as_ptr(), eta, out.f32_mut())
        });
        bridge::download(&out, dims, &device)
    }
    /// `refine_latent` with the re-noise tensor drawn on the device (`sdxl_refine_latent_seeded`)
    #[allow(clippy::too_many_arguments)]
    pub fn refine_latent_seeded(&self, latent: Tensor<B, 4>, conditioning: Conditioning<B>, unconditional_guidance_scale: f64, step_start: usize,
                                n_steps: usize, seeds: &[u64], eta: f64) -> Tensor<B, 4> {
        let device = conditioning.context_full.device();
        let dims = latent.dims();
        assert_eq!(seeds.len(), dims[0], "one seed per batch entry");
        let dc = to_c_conditioning(&conditioning);
        let d_lat = bridge::upload(latent);
        let out = DeviceBuf::new(dims.iter().product::<usize>() * 4);
        check(unsafe {
            ffi::sdxl_refine_latent_seeded(self.raw, ptr::null_mut(), d_lat.f32_ptr(), &dc.c, unconditional_guidance_scale, step_start as c_int,
                                           n_steps as c_int, seeds.as_ptr(), eta, out.f32_mut())
        });
        bridge::download(&out, dims, &device)
    }
    /// `sdxl_continue_latent` with `renoise = 0`: the handle's list (`set_sigmas`, `set_timesteps`) from `latent` as it is -- the SDXL
    /// base -> refiner handoff, the latent being what a handle whose list ends on a level returned.  `seeds` (one per batch entry) feed the
    /// `eta` noise; `None` needs `eta == 0`.  What the engine refuses is an `Err` with its message.
    pub fn continue_latent(&self, latent: Tensor<B, 4>, conditioning: Conditioning<B>, unconditional_guidance_scale: f64, n_steps: usize,
                           seeds: Option<&[u64]>, eta: f64) -> Result<Tensor<B, 4>, Box<dyn std::error::Error>> {
        let device = conditioning.context_full.device();
        let dims = latent.dims();
        if let Some(s) = seeds {
            assert_eq!(s.len(), dims[0], "one seed per batch entry");
        }
        let dc = to_c_conditioning(&conditioning);
        let d_lat = bridge::upload(latent);
        let out = DeviceBuf::new(dims.iter().product::<usize>() * 4);
        try_check(unsafe {
            ffi::sdxl_continue_latent(self.raw, ptr::null_mut(), d_lat.f32_ptr(), &dc.c, unconditional_guidance_scale, n_steps as c_int, ptr::null(),
                                      seeds.map_or(ptr::null(), |s| s.as_ptr()), eta, 0, out.f32_mut())
        })?;
        Ok(bridge::download(&out, dims, &device))
    }
    /// `gen_noise` (`:378-388`)
    fn gen_noise(conditioning: &Conditioning<B>) -> Tensor<B, 4> {
        let device = conditioning.context_full.device();
        let [n_batches, _, _] = conditioning.context_full.dims();
        let [height, width] = conditioning.resolution;
        Tensor::random([n_batches, 4, height / 8, width / 8], Distribution::Normal(0.0, 1.0), &device)
    }
    /// `Diffuser.diffusion` (`:312`): the UNet alone, reference signature of `UNet::forward` (`unet/mod.rs:450-456`)
    pub fn unet_forward(&self, x: Tensor<B, 4>, timesteps: Tensor<B, 1, Int>, context: Tensor<B, 3>, label: Tensor<B, 2>) -> Tensor<B, 4> {
        let device = x.device();
        let [b, c_in, h, w] = x.dims();
        let [_, n_ctx, _] = context.dims();
        let (d_x, (d_t, _), d_c, d_y) = (bridge::upload(x), bridge::upload_int(timesteps), bridge::upload(context), bridge::upload(label));
        let out = DeviceBuf::new(b * c_in * h * w * 4);
        let unet = unsafe { ffi::sdxl_diffuser_unet(self.raw) };
        check(unsafe {
            ffi::sdxl_unet_forward(unet, ptr::null_mut(), d_x.f32_ptr(), d_t.ptr as *const i32, d_c.f32_ptr(), d_y.f32_ptr(), b as c_int,
                                   h as c_int, w as c_int, n_ctx as c_int, out.f32_mut())
        });
        bridge::download(&out, [b, c_in, h, w], &device)
    }
    /// `unet_forward` with ControlNet residuals (`ControlNet::forward`) added at `scale` behind the middle block: `sdxl_unet_forward_residuals`.
    /// What the engine refuses (shapes that do not match, a non-finite scale, split CFG, a precision without a test) is an `Err`.
    pub fn unet_forward_residuals(&self, x: Tensor<B, 4>, timesteps: Tensor<B, 1, Int>, context: Tensor<B, 3>, label: Tensor<B, 2>,
                                  residuals: Vec<Tensor<B, 4>>, scale: f32) -> Result<Tensor<B, 4>, Box<dyn std::error::Error>> {
        let device = x.device();
        let [b, c_in, h, w] = x.dims();
        let [_, n_ctx, _] = context.dims();
        let unet = unsafe { ffi::sdxl_diffuser_unet(self.raw) };
        let mut flat: Vec<f32> = Vec::new();
        for r in residuals {
            let data: Data<f32, 4> = r.into_data().convert();
            flat.extend_from_slice(&data.value);
        }
        let d_r = DeviceBuf::from_f32(&flat);
        let (d_x, (d_t, _), d_c, d_y) = (bridge::upload(x), bridge::upload_int(timesteps), bridge::upload(context), bridge::upload(label));
        let out = DeviceBuf::new(b * c_in * h * w * 4);
        try_check(unsafe {
            ffi::sdxl_unet_forward_residuals(unet, ptr::null_mut(), d_x.f32_ptr(), d_t.ptr as *const i32, d_c.f32_ptr(), d_y.f32_ptr(), b as c_int,
                                             h as c_int, w as c_int, n_ctx as c_int, d_r.f32_ptr(), scale, out.f32_mut())
        })?;
        Ok(bridge::download(&out, [b, c_in, h, w], &device))
    }
    /// Engine options of this handle's UNet (no reference counterpart; results stay within the same tolerance class):
    /// split-CFG = the CFG pair of `forward_diffuser` (`:523-537`) as two concurrent batch-1 chains; fused cross-attention
    /// (default on) = `attn2` (`unet/mod.rs:731-795`) inside the query projection's epilogue.
    pub fn set_split_cfg(&self, enabled: bool, release_offset: usize) {
        let unet = unsafe { ffi::sdxl_diffuser_unet(self.raw) };
        check(unsafe { ffi::sdxl_unet_set_split_cfg(unet, enabled as c_int, release_offset as c_int) });
    }
    /// GroupNorm statistics from the producing convolution's epilogue (default on)
    pub fn set_gn_from_producer(&self, enabled: bool) {
        let unet = unsafe { ffi::sdxl_diffuser_unet(self.raw) };
        check(unsafe { ffi::sdxl_unet_set_gn_from_producer(unet, enabled as c_int) });
    }
    pub fn set_fused_cross_attention(&self, enabled: bool) {
        let unet = unsafe { ffi::sdxl_diffuser_unet(self.raw) };
        check(unsafe { ffi::sdxl_unet_set_fused_cross_attention(unet, enabled as c_int) });
    }
    /// GEMM classes on plain f16 operands (F32SplitMix* precisions; an F32SplitMixF16W model on parameters that are not f16 values falls back to F32SplitMix's 1 | 2 | 1024)
    pub fn mix_classes(&self) -> i32 {
        let unet = unsafe { ffi::sdxl_diffuser_unet(self.raw) };
        let mut v: c_int = 0;
        check(unsafe { ffi::sdxl_unet_mix_classes(unet, &mut v) });
        v as i32
    }
}

// ------------------------------------------------------------------------------------------------ LatentDecoder
/// `RawImages` (`stablediffusion/mod.rs:170-174`)
pub struct RawImages {
    pub buffer: Vec<Vec<u8>>,
    pub width: usize,
    pub height: usize,
}
/// `LatentDecoder<B>` (`:193-267`) over the engine's VAE; the reference runs it in f32 (`bin/sample/main.rs:121,271-278`)
pub struct LatentDecoder<B: BurnBackend> {
    raw: *mut ffi::sdxl_vae,
    _b: std::marker::PhantomData<B>,
}
impl<B: BurnBackend> Drop for LatentDecoder<B> {
    fn drop(&mut self) {
        unsafe { ffi::sdxl_vae_destroy(self.raw) };
    }
}
impl<B: BurnBackend> LatentDecoder<B> {
    pub fn synthetic(ctx: &Mi355Context, precision: Precision, seed: u64, with_encoder: bool) -> Self {
        let mut cfg: ffi::sdxl_vae_config = unsafe { std::mem::zeroed() };
        unsafe { ffi::sdxl_vae_config_default(&mut cfg) };
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::sdxl_vae_create_synthetic(ctx.raw, &cfg, precision as c_int, seed, with_encoder as c_int, &mut raw) });
        LatentDecoder { raw, _b: std::marker::PhantomData }
    }
    pub fn with_weights(ctx: &Mi355Context, precision: Precision, decoder_flat: Option<&[f32]>, encoder_flat: Option<&[f32]>)
                        -> Result<Self, Box<dyn std::error::Error>> {
        let mut cfg: ffi::sdxl_vae_config = unsafe { std::mem::zeroed() };
        unsafe { ffi::sdxl_vae_config_default(&mut cfg) };
        let mut raw = ptr::null_mut();
        try_check(unsafe {
            ffi::sdxl_vae_create(ctx.raw, &cfg, precision as c_int, decoder_flat.map_or(ptr::null(), |w| w.as_ptr()),
                                 encoder_flat.map_or(ptr::null(), |w| w.as_ptr()), &mut raw)
        })?;
        Ok(LatentDecoder { raw, _b: std::marker::PhantomData })
    }
    /// `:200-237`: the `(x+1)/2*255`, NHWC reorder, clamp and truncating u8 cast run on the device
    pub fn latent_to_image(&self, latent: Tensor<B, 4>) -> RawImages {
        let [n, _, lh, lw] = latent.dims();
        let (height, width) = (lh * 8, lw * 8);
        let d_lat = bridge::upload(latent);
        let out = DeviceBuf::new(n * height * width * 3);
        check(unsafe { ffi::sdxl_latent_to_image(self.raw, ptr::null_mut(), d_lat.f32_ptr(), n as c_int, lh as c_int, lw as c_int, out.ptr as *mut u8) });
        let flat = out.to_u8();
        let per = height * width * 3;
        RawImages { buffer: (0..n).map(|b| flat[b * per..(b + 1) * per].to_vec()).collect(), width, height }
    }
    /// `:239-255`
    pub fn image_to_latent(&self, images: &RawImages, device: &B::Device) -> Tensor<B, 4> {
        let n = images.buffer.len();
        let flat: Vec<u8> = images.buffer.iter().flatten().copied().collect();
        let d_img = DeviceBuf::from_u8(&flat);
        let dims = [n, 4, images.height / 8, images.width / 8];
        let out = DeviceBuf::new(dims.iter().product::<usize>() * 4);
        check(unsafe {
            ffi::sdxl_image_to_latent(self.raw, ptr::null_mut(), d_img.ptr as *const u8, n as c_int, images.height as c_int,
                                      images.width as c_int, out.f32_mut())
        });
        bridge::download(&out, dims, device)
    }
    /// `:257-261`
    pub fn encode_image(&self, x: Tensor<B, 4>) -> Tensor<B, 4> {
        let device = x.device();
        let [n, _, h, w] = x.dims();
        let d_x = bridge::upload(x);
        let dims = [n, 4, h / 8, w / 8];
        let out = DeviceBuf::new(dims.iter().product::<usize>() * 4);
        check(unsafe { ffi::sdxl_vae_encode_image(self.raw, ptr::null_mut(), d_x.f32_ptr(), n as c_int, h as c_int, w as c_int, out.f32_mut()) });
        bridge::download(&out, dims, &device)
    }
    /// `:263-266`
    pub fn decode_latent(&self, x: Tensor<B, 4>) -> Tensor<B, 4> {
        let device = x.device();
        let [n, _, h, w] = x.dims();
        let d_x = bridge::upload(x);
        let dims = [n, 3, 8 * h, 8 * w];
        let out = DeviceBuf::new(dims.iter().product::<usize>() * 4);
        check(unsafe { ffi::sdxl_vae_decode_latent(self.raw, ptr::null_mut(), d_x.f32_ptr(), n as c_int, h as c_int, w as c_int, out.f32_mut()) });
        bridge::download(&out, dims, &device)
    }
}

// ------------------------------------------------------------------------------------------------ Embedder
/// the reference's tokenizer trait (`src/token/mod.rs:4-11`): the host keeps its own BPE implementations
pub trait Tokenizer {
    fn encode(&self, text: &str, add_sot: bool, add_eot: bool) -> Vec<u32>;
    fn padding_token(&self) -> u32;
}
/// `Embedder<B>` (`stablediffusion/mod.rs:652-757`): both CLIP text towers run on the device, tokenisation stays host code
pub struct Embedder<B: BurnBackend, T1: Tokenizer, T2: Tokenizer> {
    ctx: *mut ffi::sdxl_ctx,
    clip: *mut ffi::sdxl_clip,
    open_clip: *mut ffi::sdxl_clip,
    clip_tokenizer: T1,
    open_clip_tokenizer: T2,
    _b: std::marker::PhantomData<B>,
}
impl<B: BurnBackend, T1: Tokenizer, T2: Tokenizer> Drop for Embedder<B, T1, T2> {
    fn drop(&mut self) {
        unsafe {
            ffi::sdxl_clip_destroy(self.clip);
            ffi::sdxl_clip_destroy(self.open_clip);
        }
    }
}
impl<B: BurnBackend, T1: Tokenizer, T2: Tokenizer> Embedder<B, T1, T2> {
    pub fn synthetic(ctx: &Mi355Context, precision: Precision, seed: u64, clip_tokenizer: T1, open_clip_tokenizer: T2) -> Self {
        let (mut c1, mut c2): (ffi::sdxl_clip_config, ffi::sdxl_clip_config) = unsafe { (std::mem::zeroed(), std::mem::zeroed()) };
        unsafe {
            ffi::sdxl_clip_config_clip_l(&mut c1);
            ffi::sdxl_clip_config_open_clip_bigg(&mut c2);
        }
        let (mut clip, mut open_clip) = (ptr::null_mut(), ptr::null_mut());
        check(unsafe { ffi::sdxl_clip_create_synthetic(ctx.raw, &c1, precision as c_int, seed, &mut clip) });
        check(unsafe { ffi::sdxl_clip_create_synthetic(ctx.raw, &c2, precision as c_int, seed + 1, &mut open_clip) });
        Embedder { ctx: ctx.raw, clip, open_clip, clip_tokenizer, open_clip_tokenizer, _b: std::marker::PhantomData }
    }
    fn tokens(tok: &dyn Tokenizer, text: &str, n_ctx: usize) -> Vec<i32> {
        // tokenize_text (`:785-801`): sot + text + eot, padded to the context length
        let mut ids: Vec<i32> = tok.encode(text, true, true).into_iter().map(|t| t as i32).collect();
        ids.truncate(n_ctx);
        ids.resize(n_ctx, tok.padding_token() as i32);
        ids
    }
    /// `tokenize_text_chunks` of the Python package: a prompt beyond the 77-token window as up to `max_chunks` (<= 4) windows.  The text is
    /// encoded without sot / eot and cut into pieces of `n_ctx - 2` ids; every piece becomes sot + piece + eot, padded with the tokenizer's pad
    /// id; at least one chunk; text beyond `max_chunks` chunks is dropped.  `max_chunks == 1` is `tokens` itself, truncation included.  The
    /// chunks are encoded as batch rows (`sdxl_clip_forward_hidden(tower, ids, c, 77, ..)`), concatenated along the token axis (`[c, 77, n]` is
    /// `[77 c, n]` in memory), the pooled embedding is chunk 0's, and the UNet is given `n_ctx = 77 c` for both contexts.
    pub fn tokens_chunked(tok: &dyn Tokenizer, text: &str, n_ctx: usize, max_chunks: usize) -> Vec<Vec<i32>> {
        assert!((1..=4).contains(&max_chunks), "max_chunks must be 1 .. 4");
        if max_chunks == 1 {
            return vec![Self::tokens(tok, text, n_ctx)];
        }
        let ids: Vec<i32> = tok.encode(text, false, false).into_iter().map(|t| t as i32).collect();
        let n = n_ctx - 2;
        let mut pieces: Vec<&[i32]> = ids.chunks(n).take(max_chunks).collect();
        if pieces.is_empty() {
            pieces.push(&[]);
        }
        let (sot, eot) = (tok.encode("", true, false)[0] as i32, tok.encode("", false, true)[0] as i32);
        pieces.iter().map(|p| {
            let mut c = Vec::with_capacity(n_ctx);
            c.push(sot);
            c.extend_from_slice(p);
            c.push(eot);
            c.resize(n_ctx, tok.padding_token() as i32);
            c
        }).collect()
    }
    /// one prompt -- its `rows` chunks of 77 ids as batch rows -- through one tower: (penultimate hidden state [rows * 77, n_state]: the chunks side by
    /// side along the token axis; pooled projection [embed_dim] of chunk 0 when asked for)
    fn run_tower(&self, tower: *mut ffi::sdxl_clip, ids: &[i32], rows: usize, n_state: usize, embed_dim: usize, hidden_idx: i32, pooled: bool) -> (Vec<f32>, Vec<f32>) {
        let seq = ids.len() / rows;
        let d_ids = DeviceBuf::new(ids.len() * 4);
        assert_eq!(unsafe { hipMemcpy(d_ids.ptr, ids.as_ptr() as *const c_void, ids.len() * 4, HIP_MEMCPY_HOST_TO_DEVICE) }, 0);
        let hidden = DeviceBuf::new(ids.len() * n_state * 4);
        let pool = DeviceBuf::new(rows * embed_dim * 4);
        if pooled {
            check(unsafe {
                ffi::sdxl_clip_forward_hidden_pooled(tower, ptr::null_mut(), d_ids.ptr as *const i32, rows as c_int, seq as c_int, hidden_idx,
                                                     hidden.f32_mut(), pool.f32_mut())
            });
        } else {
            check(unsafe { ffi::sdxl_clip_forward_hidden(tower, ptr::null_mut(), d_ids.ptr as *const i32, rows as c_int, seq as c_int, hidden_idx, hidden.f32_mut()) });
        }
        let mut p = pool.to_f32();
        p.truncate(embed_dim);
        (hidden.to_f32(), p)
    }
    /// reference signature (`:661-667`)
    pub fn text_to_conditioning(&self, text: &str, size: Tensor<B, 2, Int>, crop: Tensor<B, 2, Int>, ar: Tensor<B, 1, Int>) -> Conditioning<B> {
        self.text_to_conditioning_chunked(text, "", 1, size, crop, ar)
    }
    /// `Embedder.text_to_conditioning(text, size, crop, ar, negative=, max_chunks=)` of the Python package: a negative prompt, and prompts beyond
    /// the 77-token window as up to `max_chunks` (<= 4) chunks.  `c` = the largest chunk count among the four tokenisations; shorter ones are filled
    /// with chunks of the empty prompt, so that both contexts have 77 c tokens.  `("", 1)` is the reference's call.
    pub fn text_to_conditioning_chunked(&self, text: &str, negative: &str, max_chunks: usize, size: Tensor<B, 2, Int>, crop: Tensor<B, 2, Int>,
                                        ar: Tensor<B, 1, Int>) -> Conditioning<B> {
        let device = size.device();
        let ar_v: Vec<i64> = ar.clone().into_data().value.iter().map(|x| x.elem::<i64>()).collect();
        let resolution = [ar_v[0] as usize, ar_v[1] as usize];
        const CHUNK: usize = 77;
        let chunks = |tok: &dyn Tokenizer, t: &str| Self::tokens_chunked(tok, t, CHUNK, max_chunks);
        let mut ids = [chunks(&self.clip_tokenizer, text), chunks(&self.open_clip_tokenizer, text),
                       chunks(&self.clip_tokenizer, negative), chunks(&self.open_clip_tokenizer, negative)];
        let c = ids.iter().map(|v| v.len()).max().unwrap();
        for (i, v) in ids.iter_mut().enumerate() {
            let tok: &dyn Tokenizer = if i % 2 == 0 { &self.clip_tokenizer as &dyn Tokenizer } else { &self.open_clip_tokenizer as &dyn Tokenizer };
            while v.len() < c {
                v.push(Self::tokens(tok, "", CHUNK));
            }
        }
        let n_ctx = CHUNK * c;
        // CLIP-L: hidden state after 11 of 12 blocks; OpenCLIP bigG: after 31 of 32 + pooled text embedding (`:676-688`)
        let embed = |clip_ids: &Vec<Vec<i32>>, open_ids: &Vec<Vec<i32>>| {
            let (h1, _) = self.run_tower(self.clip, &clip_ids.concat(), c, 768, 768, 11, false);
            let (h2, pooled) = self.run_tower(self.open_clip, &open_ids.concat(), c, 1280, 1280, 31, true);
            let mut full = Vec::with_capacity(n_ctx * 2048);
            for t in 0..n_ctx {
                full.extend_from_slice(&h1[t * 768..(t + 1) * 768]);
                full.extend_from_slice(&h2[t * 1280..(t + 1) * 1280]);
            }
            (full, h2, pooled)
        };
        let (full, open, pooled) = embed(&ids[0], &ids[1]);
        let (ufull, uopen, upooled) = embed(&ids[2], &ids[3]);
        // conditioning_embedding (`unet/mod.rs:41-57`): pooled | sinusoid(size, crop, ar); the refiner variant swaps ar for
        // the aesthetic score 6 (`stablediffusion/mod.rs:709,740`)
        let ints = |t: Tensor<B, 2, Int>| -> Vec<i32> { t.into_data().value.iter().map(|x| x.elem::<i32>()).collect() };
        let (size_v, crop_v) = (ints(size), ints(crop));
        let cond_emb = |pooled: &[f32], vals: &[i32]| -> Vec<f32> {
            let (d_p, d_v) = (DeviceBuf::from_f32(pooled), DeviceBuf::new(vals.len() * 4));
            assert_eq!(unsafe { hipMemcpy(d_v.ptr, vals.as_ptr() as *const c_void, vals.len() * 4, HIP_MEMCPY_HOST_TO_DEVICE) }, 0);
            let out = DeviceBuf::new((pooled.len() + vals.len() * 256) * 4);
            check(unsafe {
                ffi::sdxl_conditioning_embedding(self.ctx, ptr::null_mut(), d_p.f32_ptr(), 1, pooled.len() as c_int, d_v.ptr as *const i32,
                                                 vals.len() as c_int, 256, out.f32_mut())
            });
            out.to_f32()
        };
        let base_vals: Vec<i32> = [&size_v[..2], &crop_v[..2], &[ar_v[0] as i32, ar_v[1] as i32][..]].concat();
        let refiner_vals: Vec<i32> = [&size_v[..2], &crop_v[..2], &[6][..]].concat();
        let t2 = |v: Vec<f32>, c: usize| Tensor::<B, 2>::from_data(Data::new(v, Shape::new([n_ctx, c])).convert(), &device);
        let t1 = |v: Vec<f32>| { let n = v.len(); Tensor::<B, 1>::from_data(Data::new(v, Shape::new([n])).convert(), &device) };
        Conditioning {
            unconditional_context_full: t2(ufull, 2048),
            unconditional_context_open_clip: t2(uopen, 1280),
            context_full: t2(full, 2048).unsqueeze(),
            context_open_clip: t2(open, 1280).unsqueeze(),
            unconditional_channel_context: t1(cond_emb(&upooled, &base_vals)),
            unconditional_channel_context_refiner: t1(cond_emb(&upooled, &refiner_vals)),
            channel_context: t1(cond_emb(&pooled, &base_vals)).unsqueeze(),
            channel_context_refiner: t1(cond_emb(&pooled, &refiner_vals)).unsqueeze(),
            resolution,
        }
    }
}

// ------------------------------------------------------------------------------------------------ operator plug-in
/// the reference's own operator plug-in point (`src/backend.rs:3-24`).  Same trait, same default bodies; a backend opts into
/// the MI355X kernels by overriding the two methods with the functions below, exactly as the reference overrides them for
/// `LibTorch<E>` (`src/backend.rs:31-80`).
pub trait Backend: BurnBackend {
    fn qkv_attention(q: Self::FloatTensorPrimitive<3>, k: Self::FloatTensorPrimitive<3>, v: Self::FloatTensorPrimitive<3>,
                     mask: Option<Self::FloatTensorPrimitive<2>>, n_head: usize) -> Self::FloatTensorPrimitive<3> {
        mi355_qkv_attention::<Self>(Tensor::from_primitive(q), Tensor::from_primitive(k), Tensor::from_primitive(v),
                                    mask.map(Tensor::from_primitive), n_head)
            .into_primitive()
    }
    fn attn_decoder_mask(seq_length: usize, device: &Self::Device) -> Self::FloatTensorPrimitive<2> {
        mi355_attn_decoder_mask::<Self>(seq_length, device).into_primitive()
    }
}
thread_local! {
    /// the context the operator plug-in launches on (the trait's functions are static: no `self` to carry it)
    static OP_CTX: std::cell::RefCell<Option<Mi355Context>> = const { std::cell::RefCell::new(None) };
}
fn with_op_ctx<R>(f: impl FnOnce(*mut ffi::sdxl_ctx) -> R) -> R {
    OP_CTX.with(|c| {
        let mut c = c.borrow_mut();
        if c.is_none() {
            *c = Some(Mi355Context::new(0).expect("sdxl_mi355: no MI355X visible (the engine has no CPU path)"));
        }
        f(c.as_ref().unwrap().raw)
    })
}
/// `qkv_attention` (`src/backend.rs:88-128`): q [B,Nq,C], k/v [B,Nk,C], additive mask [Nq,Nk] -> [B,Nq,C]
pub fn mi355_qkv_attention<B: BurnBackend>(q: Tensor<B, 3>, k: Tensor<B, 3>, v: Tensor<B, 3>, mask: Option<Tensor<B, 2>>, n_head: usize) -> Tensor<B, 3> {
    let device = q.device();
    let [b, nq, c] = q.dims();
    let [_, nk, _] = k.dims();
    let (d_q, d_k, d_v) = (bridge::upload(q), bridge::upload(k), bridge::upload(v));
    let d_m = mask.map(|m| bridge::upload(m.slice([0..nq, 0..nk])));
    let out = DeviceBuf::new(b * nq * c * 4);
    with_op_ctx(|ctx| {
        check(unsafe {
            ffi::sdxl_qkv_attention(ctx, ptr::null_mut(), d_q.f32_ptr(), d_k.f32_ptr(), d_v.f32_ptr(), d_m.as_ref().map_or(ptr::null(), |m| m.f32_ptr()),
                                    b as c_int, nq as c_int, nk as c_int, c as c_int, n_head as c_int, ffi::SDXL_DTYPE_F32 as c_int, out.f32_mut())
        })
    });
    bridge::download(&out, [b, nq, c], &device)
}
/// `attn_decoder_mask` (`src/backend.rs:130-136`)
pub fn mi355_attn_decoder_mask<B: BurnBackend>(seq_length: usize, device: &B::Device) -> Tensor<B, 2> {
    let out = DeviceBuf::new(seq_length * seq_length * 4);
    with_op_ctx(|ctx| check(unsafe { ffi::sdxl_attn_decoder_mask(ctx, ptr::null_mut(), seq_length as c_int, out.f32_mut()) }));
    bridge::download(&out, [seq_length, seq_length], device)
}
