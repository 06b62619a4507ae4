// Replacement bodies for the reference's per-node pixel functions, written against
// kanter_core_amd_sys.rs.  SOURCE ONLY: there is no Rust toolchain in this build environment, so
// this file has never been compiled; it shows exactly where the C ABI plugs into vismut_core 0.10.0
// (paths and line numbers refer to the reference checkout).  The public API of the crate
// (NodeGraph / LiveGraph / TextureProcessor / Node / SlotData) does not change.
//
// Drop-in points:
//   src/slot_image.rs   SlotImage keeps its two variants but wraps a device image handle
//   src/node/mix.rs:51            mix::process
//   src/node/separate_rgba.rs:38  separate_rgba::process
//   src/node/combine_rgba.rs:14   combine_rgba::process
//   src/node/value.rs:14          value::process
//   src/node/height_to_normal.rs:16  height_to_normal::process
//   src/shared.rs:16,141,218      deconstruct_image / resize_buffers / read_slot_image
//   src/slot_image.rs:28,146,172,212  from_value / to_u8 / to_u8_srgb / as_type
use crate::kanter_core_amd_sys::*;
use crate::{edge::Edge, error::{Result, TexProError}, node::{mix::MixType, Node, ResizeFilter, ResizePolicy},
            node_graph::SlotId, slot_data::{Size, SlotData}};
use std::{ffi::CStr, os::raw::c_void, ptr, sync::Arc};

/// Owned reference to a device image (kc_image is reference counted by the library).
pub struct DeviceImage(ptr::NonNull<KcImage>);
unsafe impl Send for DeviceImage {}
unsafe impl Sync for DeviceImage {}
impl Clone for DeviceImage {
    fn clone(&self) -> Self { unsafe { kc_image_retain(self.0.as_ptr()) }; DeviceImage(self.0) }
}
impl Drop for DeviceImage {
    fn drop(&mut self) { unsafe { kc_image_release(self.0.as_ptr()) }; }
}

/// src/slot_image.rs:15-19 -- same two variants, planes live in HBM.
#[derive(Clone)]
pub enum SlotImage { Gray(DeviceImage), Rgba(DeviceImage) }

fn check(status: i32) -> Result<()> {
    // 1..=19 are TexProError in declaration order (src/error.rs:5-27); the two variants that carry a payload are built
    // from kc_last_error() (the library keeps the text, not the foreign error object); >= 100 are the library's own.
    let text = || unsafe { CStr::from_ptr(kc_last_error()) }.to_string_lossy().into_owned();
    match status {
        0 => Ok(()),
        1 => Err(TexProError::Generic),
        2 => Err(TexProError::Canceled),
        3 => Err(TexProError::Image(image::ImageError::IoError(std::io::Error::new(std::io::ErrorKind::Other, text())))),
        4 => Err(TexProError::InvalidBufferCount),
        5 => Err(TexProError::InvalidNodeId),
        6 => Err(TexProError::InvalidNodeType),
        7 => Err(TexProError::InvalidSlotId),
        8 => Err(TexProError::InvalidSlotType),
        9 => Err(TexProError::InvalidEdge),
        10 => Err(TexProError::NoSlotData),
        11 => Err(TexProError::SlotOccupied),
        12 => Err(TexProError::SlotNotOccupied),
        13 => Err(TexProError::UnableToLock),
        14 => Err(TexProError::NodeProcessing),
        15 => Err(TexProError::PoisonError),
        16 => Err(TexProError::TryLockError),
        17 => Err(TexProError::NodeDirty),
        18 => Err(TexProError::Io(std::io::Error::new(std::io::ErrorKind::Other, text()))),
        19 => Err(TexProError::InvalidName),
        _ => {
            // KC_ERR_HIP / NO_DEVICE / INVALID_ARG / OUT_OF_MEMORY / UNSUPPORTED: no counterpart in the reference
            eprintln!("kanter_core_amd: status {}: {}", status, text());
            Err(TexProError::Generic)
        }
    }
}

fn wrap(raw: *mut KcImage) -> SlotImage {
    let img = DeviceImage(ptr::NonNull::new(raw).expect("null image"));
    let mut rgba = 0;
    unsafe { kc_image_is_rgba(raw, &mut rgba) };
    if rgba != 0 { SlotImage::Rgba(img) } else { SlotImage::Gray(img) }
}

impl SlotImage {
    fn raw(&self) -> *mut KcImage { match self { Self::Gray(i) | Self::Rgba(i) => i.0.as_ptr() } }
    pub fn is_rgba(&self) -> bool { matches!(self, Self::Rgba(_)) }

    /// src/slot_image.rs:116-121
    pub fn size(&self) -> Result<Size> {
        let mut s = KcSize { width: 0, height: 0 };
        check(unsafe { kc_image_size(self.raw(), &mut s) })?;
        Ok(Size::new(s.width, s.height))
    }
    /// src/slot_image.rs:28-64
    pub fn from_value(size: Size, value: f32, rgba: bool) -> Self {
        let mut out = ptr::null_mut();
        let s = KcSize { width: size.width, height: size.height };
        check(unsafe { kc_image_from_value(s, value, rgba as i32, &mut out) }).unwrap();
        wrap(out)
    }
    /// src/slot_image.rs:212-256
    pub fn as_type(&self, rgba: bool) -> Result<Self> {
        let mut out = ptr::null_mut();
        check(unsafe { kc_image_as_type(self.raw(), rgba as i32, &mut out) })?;
        Ok(wrap(out))
    }
    /// src/slot_image.rs:146-170 (srgb = true: :172-207)
    fn to_u8_impl(&self, srgb: bool) -> Result<Vec<u8>> {
        let s = self.size()?;
        let mut v = vec![0u8; s.pixel_count() * 4];
        check(unsafe { kc_image_to_u8(self.raw(), srgb as i32, v.as_mut_ptr()) })?;
        Ok(v)
    }
    pub fn to_u8(&self) -> Result<Vec<u8>> { self.to_u8_impl(false) }
    pub fn to_u8_srgb(&self) -> Result<Vec<u8>> { self.to_u8_impl(true) }
    /// Per-channel min / max / NaN count, and with `histogram` the bins to_u8 (`srgb`: to_u8_srgb) writes, computed on the
    /// device (kc_image_channel_stats); only the first `channels` entries of each array describe the image.
    pub fn channel_stats(&self, histogram: bool, srgb: bool) -> Result<Box<KcChannelStats>> {
        let flags = if histogram { KC_STATS_HISTOGRAM } else { 0 } | if srgb { KC_STATS_SRGB } else { 0 };
        // about 8 KiB: on the heap; every field is plain data, so all-zero bytes are a valid value
        let mut out: Box<KcChannelStats> = Box::new(unsafe { std::mem::zeroed() });
        check(unsafe { kc_image_channel_stats(self.raw(), flags, &mut *out) })?;
        Ok(out)
    }
    /// The signed distance field of a cutout, for alpha-tested magnification (kc_image_distance_field): a new Gray image in which
    /// every texel holds 0.5 + sd / (2 spread), sd its exact distance in texels to the boundary of the mask "to_u8 writes
    /// `channel` (None: alpha of an RGBA image, the value of a Gray one) as at least `ref_u8`", positive inside, saturating at 0
    /// and 1 beyond `spread` (1..KC_SDF_MAX_SPREAD) texels.  `tiles`: the image tiles on both axes (KC_SDF_WRAP).
    pub fn distance_field(&self, ref_u8: u8, spread: u32, channel: Option<u32>, tiles: bool) -> Result<Self> {
        let ch = channel.unwrap_or(if self.is_rgba() { 3 } else { 0 });
        let mut out = ptr::null_mut();
        check(unsafe { kc_image_distance_field(self.raw(), ch, ref_u8 as u32, spread, if tiles { KC_SDF_WRAP } else { 0 }, &mut out) })?;
        Ok(wrap(out))
    }
    /// A separable Gaussian blur of the image's planes (kc_image_blur): a new image of this type and size, exact as a function
    /// of its f32 weights (kc_blur_weights, kc_blur_texel).  A sigma of 0 leaves its axis alone; the radius max(1, ceil(3 sigma))
    /// goes up to KC_BLUR_MAX_RADIUS.  Edges repeat; `tiles`: the image tiles on both axes (KC_BLUR_WRAP).  Bit c of
    /// `channel_mask` (None: every channel) selects channel c; the other channels are this image's own planes.
    pub fn blur(&self, sigma_x: f32, sigma_y: f32, channel_mask: Option<u32>, tiles: bool) -> Result<Self> {
        let mask = channel_mask.unwrap_or(if self.is_rgba() { 15 } else { 1 });
        let mut out = ptr::null_mut();
        check(unsafe { kc_image_blur(self.raw(), sigma_x, sigma_y, mask, if tiles { KC_BLUR_WRAP } else { 0 }, &mut out) })?;
        Ok(wrap(out))
    }
    /// The image's BC1, BC3, BC4, BC5 or BC7 blocks (kc_image_to_bc), encoded on the device from the bytes to_u8 (`srgb`:
    /// to_u8_srgb, BC1, BC3 and BC7 only) writes: ceil(h/4) rows of ceil(w/4) blocks of 8 (BC1, BC4) or 16 (BC3, BC5, BC7) bytes,
    /// tightly packed.
    pub fn to_bc(&self, format: i32, srgb: bool) -> Result<Vec<u8>> {
        let s = self.size()?;
        let block = if format == KC_BC1 || format == KC_BC4 { 8 } else { 16 };
        let mut out = vec![0u8; ((s.width as usize + 3) / 4) * ((s.height as usize + 3) / 4) * block];
        let flags = if srgb { KC_BC_SRGB } else { 0 };
        check(unsafe { kc_image_to_bc(self.raw(), format, flags, out.as_mut_ptr(), out.len()) })?;
        Ok(out)
    }
    /// The BC blocks of the whole mip chain (kc_image_to_bc_mips): level k is max(1, w >> k) by max(1, h >> k), the 2 x 2 box of
    /// the level above it in f32, built on the device; the levels follow one another, tightly packed, down to 1 x 1.  Returns the
    /// bytes and the offset of every level (kc_bc_mip_layout).
    pub fn to_bc_mips(&self, format: i32, srgb: bool) -> Result<(Vec<u8>, Vec<usize>)> {
        self.bc_mips_with(format, if srgb { KC_BC_SRGB } else { 0 })
    }
    /// to_bc_mips of a normal map (KC_MIP_NORMALS; KC_BC5 is the usual format): R, G, B are a vector stored as n * 0.5 + 0.5 and
    /// every level is renormalised on the device before the next is made, so the coarser levels do not flatten.
    pub fn to_normal_bc_mips(&self, format: i32) -> Result<(Vec<u8>, Vec<usize>)> {
        self.bc_mips_with(format, KC_MIP_NORMALS)
    }
    /// to_bc_mips of an alpha-tested cutout (KC_MIP_COVERAGE_REF; KC_BC3 and KC_BC7 carry alpha): every level's alpha is rescaled
    /// on the device so that the share of texels a renderer's test against the byte `reference` (1..=255) keeps stays level 0's.
    pub fn to_cutout_bc_mips(&self, format: i32, srgb: bool, reference: u8) -> Result<(Vec<u8>, Vec<usize>)> {
        self.bc_mips_with(format, kc_mip_coverage_ref(reference) | if srgb { KC_BC_SRGB } else { 0 })
    }
    fn bc_mips_with(&self, format: i32, flags: u32) -> Result<(Vec<u8>, Vec<usize>)> {
        let s = self.size()?;
        let (mut levels, mut total) = (0u32, 0usize);
        check(unsafe { kc_bc_mip_layout(s.width, s.height, format, &mut levels, ptr::null_mut(), 0, &mut total) })?;
        let mut offsets = vec![0usize; levels as usize];
        check(unsafe { kc_bc_mip_layout(s.width, s.height, format, &mut levels, offsets.as_mut_ptr(), levels, &mut total) })?;
        let mut out = vec![0u8; total];
        check(unsafe { kc_image_to_bc_mips(self.raw(), format, flags, out.as_mut_ptr(), out.len()) })?;
        Ok((out, offsets))
    }
    /// The mip level a preview of at most `max_extent` texels a side is cut from (kc_preview_level): (level, its size).  No device.
    pub fn preview_level(size: Size, max_extent: u32) -> Result<(u32, Size)> {
        let (mut level, mut w, mut h) = (0u32, 0u32, 0u32);
        check(unsafe { kc_preview_level(size.width, size.height, max_extent, &mut level, &mut w, &mut h) })?;
        Ok((level, Size::new(w, h)))
    }
    /// RGBA8 rects of mip levels of many images in one call (kc_image_previews), without building a chain: each request is
    /// (image, level, rect (x, y, width, height) in texels of that level, None = the whole level).  Returns one tightly packed
    /// width * height * 4 byte vector per request: to_u8 (`srgb`: to_u8_srgb) of that level of the chain, cut to the rect.
    pub fn previews(requests: &[(&SlotImage, u32, Option<(u32, u32, u32, u32)>)], srgb: bool) -> Result<Vec<Vec<u8>>> {
        let mut reqs = Vec::with_capacity(requests.len());
        let mut total = 0usize;
        for (img, level, rect) in requests {
            let s = img.size()?;
            let (x, y, w, h) = rect.unwrap_or((0, 0, s.width.checked_shr(*level).unwrap_or(0).max(1), s.height.checked_shr(*level).unwrap_or(0).max(1)));
            reqs.push(KcPreviewRequest { image: img.raw(), level: *level, x, y, width: w, height: h, offset_bytes: total,
                                         row_pitch_bytes: w as usize * 4 });
            total += w as usize * h as usize * 4;
        }
        let mut out = vec![0u8; total.max(4)];
        let flags = if srgb { KC_PREVIEW_SRGB } else { 0 };
        check(unsafe { kc_image_previews(reqs.as_ptr(), reqs.len() as u32, flags, out.as_mut_ptr(), out.len()) })?;
        Ok(reqs.iter().map(|q| out[q.offset_bytes..q.offset_bytes + q.width as usize * q.height as usize * 4].to_vec()).collect())
    }
    /// The image that tightly packed BC blocks decode to (kc_image_from_bc), decoded on the device: to_u8 of the result is exactly
    /// the decoded bytes.  `gray` (BC4 only): a Gray image of the channel.  Also returns the BC7 blocks of partitioned modes,
    /// which are not decoded and give (0, 0, 0, 0).
    pub fn from_bc(blocks: &[u8], size: Size, format: i32, gray: bool) -> Result<(Self, u64)> {
        let (mut out, mut undecoded) = (ptr::null_mut(), 0u64);
        let flags = if gray { KC_BC_GRAY } else { 0 };
        check(unsafe { kc_image_from_bc(blocks.as_ptr(), blocks.len(), size.width, size.height, format, flags, &mut out, &mut undecoded) })?;
        Ok((wrap(out), undecoded))
    }
    /// How far the image's BC encoding is from the image (kc_image_bc_error): the decoded bytes against the bytes to_u8 (`srgb`:
    /// to_u8_srgb) writes, summed over the image's pixels on the device.
    pub fn bc_error(&self, format: i32, srgb: bool) -> Result<KcBcError> {
        let mut out: KcBcError = unsafe { std::mem::zeroed() };
        check(unsafe { kc_image_bc_error(self.raw(), format, if srgb { KC_BC_SRGB } else { 0 }, &mut out) })?;
        Ok(out)
    }
    /// Level `level` of a .dds file of BC blocks, decoded as from_bc (kc_image_read_dds), and what its header says.
    pub fn read_dds(path: &std::path::Path, level: u32, gray: bool) -> Result<(Self, KcDdsInfo)> {
        let c = std::ffi::CString::new(path.to_string_lossy().as_bytes()).map_err(|_| TexProError::Generic)?;
        let (mut out, mut info): (*mut KcImage, KcDdsInfo) = (ptr::null_mut(), unsafe { std::mem::zeroed() });
        check(unsafe { kc_image_read_dds(c.as_ptr(), level, if gray { KC_BC_GRAY } else { 0 }, &mut out, &mut info) })?;
        Ok((wrap(out), info))
    }
}

/// src/shared.rs:218-261 (decode with the `image` crate as before, then hand the u8 samples over).
pub fn read_slot_image<P: AsRef<std::path::Path>>(path: P) -> Result<SlotImage> {
    let image = ::image::open(path)?;
    let px = image.as_flat_samples_u8().unwrap().samples;
    let (w, h) = (image.width(), image.height());
    let channels = (px.len() / (w * h) as usize) as i32;
    let mut out = ptr::null_mut();
    check(unsafe { kc_image_from_u8(px.as_ptr(), w, h, channels, &mut out) })?;
    Ok(wrap(out))
}

fn slot(slot_datas: &[Arc<SlotData>], id: u32) -> *mut KcImage {
    slot_datas.iter().find(|sd| sd.slot_id == SlotId(id)).map_or(ptr::null_mut(), |sd| sd.image.raw())
}

/// src/node/mix.rs:51-134
pub(crate) fn mix_process(slot_datas: &[Arc<SlotData>], node: &Node, mix_type: MixType) -> Result<Vec<Arc<SlotData>>> {
    let mut out = ptr::null_mut();
    check(unsafe { kc_mix_process(slot(slot_datas, 0), slot(slot_datas, 1), mix_type as i32, &mut out) })?;
    Ok(if out.is_null() { Vec::new() } else { vec![Arc::new(SlotData::new(node.node_id, SlotId(0), wrap(out)))] })
}

/// src/node/separate_rgba.rs:38-69
pub(crate) fn separate_rgba_process(slot_datas: &[Arc<SlotData>], node: &Node) -> Result<Vec<Arc<SlotData>>> {
    let input = slot_datas.get(0).map_or(ptr::null_mut(), |sd| sd.image.raw());
    let mut outs = [ptr::null_mut(); 4];
    check(unsafe { kc_separate_rgba_process(input, outs.as_mut_ptr()) })?;
    Ok(outs.iter().enumerate().map(|(i, o)| Arc::new(SlotData::new(node.node_id, SlotId(i as u32), wrap(*o)))).collect())
}

/// src/node/combine_rgba.rs:14-97
pub(crate) fn combine_rgba_process(slot_datas: &[Arc<SlotData>], node: &Node) -> Result<Vec<Arc<SlotData>>> {
    let ins = [slot(slot_datas, 0), slot(slot_datas, 1), slot(slot_datas, 2), slot(slot_datas, 3)];
    let mut out = ptr::null_mut();
    check(unsafe { kc_combine_rgba_process(ins.as_ptr(), &mut out) })?;
    Ok(vec![Arc::new(SlotData::new(node.node_id, SlotId(0), wrap(out)))])
}

/// src/node/value.rs:14-26
pub(crate) fn value_process(node: &Node, value: f32) -> Vec<Arc<SlotData>> {
    let mut out = ptr::null_mut();
    check(unsafe { kc_value_process(value, &mut out) }).unwrap();
    vec![Arc::new(SlotData::new(node.node_id, SlotId(0), wrap(out)))]
}

/// src/node/height_to_normal.rs:16-77 (a 100 us kernel: the per-pixel cancel poll has no analogue)
pub(crate) fn height_to_normal_process(slot_datas: &[Arc<SlotData>], node: &Node) -> Result<Vec<Arc<SlotData>>> {
    let mut out = ptr::null_mut();
    check(unsafe { kc_height_to_normal_process(slot(slot_datas, 0), &mut out) })?;
    Ok(if out.is_null() { Vec::new() } else { vec![Arc::new(SlotData::new(node.node_id, SlotId(0), wrap(out)))] })
}

/// src/shared.rs:141-216 -- `edges` already sorted by input_slot (src/node/node_type.rs:230-231).
pub(crate) fn resize_buffers(slot_datas: &[Arc<SlotData>], edges: &[Edge], policy: ResizePolicy, filter: ResizeFilter)
    -> Result<Vec<Arc<SlotData>>> {
    if slot_datas.is_empty() { return Ok(slot_datas.into()); }
    let images: Vec<*mut KcImage> = slot_datas.iter().map(|sd| sd.image.raw()).collect();
    let key = |n: u32, s: u32| KcEdge { output_id: n, input_id: 0, output_slot: s, input_slot: 0 };
    let keys: Vec<KcEdge> = slot_datas.iter().map(|sd| key(sd.node_id.0, sd.slot_id.0)).collect();
    let es: Vec<KcEdge> = edges.iter().map(|e| KcEdge { output_id: e.output_id.0, input_id: e.input_id.0,
                                                        output_slot: e.output_slot.0, input_slot: e.input_slot.0 }).collect();
    let (p, pslot, psize) = match policy {
        ResizePolicy::MostPixels => (0, 0, KcSize { width: 0, height: 0 }),
        ResizePolicy::LeastPixels => (1, 0, KcSize { width: 0, height: 0 }),
        ResizePolicy::LargestAxes => (2, 0, KcSize { width: 0, height: 0 }),
        ResizePolicy::SmallestAxes => (3, 0, KcSize { width: 0, height: 0 }),
        ResizePolicy::SpecificSlot(s) => (4, s.0, KcSize { width: 0, height: 0 }),
        ResizePolicy::SpecificSize(s) => (5, 0, KcSize { width: s.width, height: s.height }),
    };
    let mut outs = vec![ptr::null_mut(); images.len()];
    check(unsafe { kc_resize_buffers(images.as_ptr(), keys.as_ptr(), images.len() as i32, es.as_ptr(), es.len() as i32,
                                     p, pslot, psize, filter as i32, outs.as_mut_ptr()) })?;
    Ok(slot_datas.iter().zip(outs).map(|(sd, o)| Arc::new(SlotData::new(sd.node_id, sd.slot_id, wrap(o)))).collect())
}

// ------------------------------------------------------------------------------------------------
// Several GPUs (one process per GPU).  The reference has no such layer; these are the calls a Rust host adds
// around `LiveGraph`: join the communicator once, make a plan, evaluate it.  The library moves the data itself
// (csrc/comm.cpp); INTEGRATION.md section 6 shows the whole sequence.
// ------------------------------------------------------------------------------------------------

/// How the evaluation of one node is spread over the ranks (kc_live_graph_partition, csrc/partition.cpp): the same answer
/// on every rank, derived from the graph alone.  Owns the library's plan.
pub struct Plan {
    raw: *mut KcPartition,
    /// 0 = one GPU, 1 = branches (`transfers` cross rank boundaries), 2 = row bands (`bands`)
    pub kind: i32,
    pub nodes: Vec<KcPlacement>,
    pub transfers: Vec<KcTransfer>,
    /// rows [y0, y1) of the requested node per rank (band plans)
    pub bands: Vec<KcBandRange>,
}

impl Drop for Plan {
    fn drop(&mut self) { unsafe { kc_partition_free(self.raw); } }
}

/// rank 0: the identifier every rank passes to `comm_init` (hand it over by any channel the host has)
pub fn comm_unique_id() -> Result<[u8; 256]> {
    let mut id = [0u8; 256];
    check(unsafe { kc_comm_unique_id(id.as_mut_ptr() as *mut c_void) })?;
    Ok(id)
}

/// collective over all ranks of the node, after `kc_init`
pub fn comm_init(rank: i32, world: i32, id: &[u8; 256]) -> Result<()> {
    check(unsafe { kc_comm_init(rank, world, id.as_ptr() as *const c_void) })
}

pub fn comm_destroy() -> Result<()> { check(unsafe { kc_comm_destroy() }) }

/// policy: 0 = the cheapest of {one GPU, branches, row bands + gather}, 1 = branches, 2 = row bands
pub fn partition(lg: *mut KcLiveGraph, root: NodeId, world: i32, policy: i32) -> Result<Plan> {
    let mut raw = ptr::null_mut();
    check(unsafe { kc_live_graph_partition(lg, root.0, world, policy, &mut raw) })?;
    let mut plan = Plan { raw, kind: 0, nodes: Vec::new(), transfers: Vec::new(), bands: Vec::new() };
    check(unsafe { kc_partition_kind(raw, &mut plan.kind, ptr::null_mut(), ptr::null_mut(), ptr::null_mut()) })?;
    let (mut n, mut t, mut b) = (0u32, 0u32, 0u32);
    check(unsafe { kc_partition_nodes(raw, ptr::null_mut(), 0, &mut n) })?;
    check(unsafe { kc_partition_transfers(raw, ptr::null_mut(), 0, &mut t) })?;
    check(unsafe { kc_partition_bands(raw, ptr::null_mut(), 0, &mut b, ptr::null_mut(), ptr::null_mut()) })?;
    plan.nodes = vec![KcPlacement { node_id: 0, rank: 0, component: 0, kind: 0 }; n as usize];
    plan.transfers = vec![KcTransfer { node_id: 0, slot_id: 0, src_rank: 0, dst_rank: 0, level: 0 }; t as usize];
    plan.bands = vec![KcBandRange { y0: 0, y1: 0 }; b as usize];
    check(unsafe { kc_partition_nodes(raw, plan.nodes.as_mut_ptr(), n, &mut n) })?;
    check(unsafe { kc_partition_transfers(raw, plan.transfers.as_mut_ptr(), t, &mut t) })?;
    check(unsafe { kc_partition_bands(raw, plan.bands.as_mut_ptr(), b, &mut b, ptr::null_mut(), ptr::null_mut()) })?;
    Ok(plan)
}

/// The whole evaluation of a plan (kc_live_graph_evaluate_partitioned): the exchange of a branch plan and the root on the
/// home rank, or this rank's rows of a band plan and the gather.  `Some(image)` on the home rank, `None` elsewhere.
pub fn evaluate_partitioned(lg: *mut KcLiveGraph, plan: &Plan, root: NodeId) -> Result<Option<SlotImage>> {
    let mut out = ptr::null_mut();
    check(unsafe { kc_live_graph_evaluate_partitioned(lg, plan.raw, root.0, &mut out) })?;
    Ok(if out.is_null() { None } else { Some(wrap(out)) })
}

/// Every rank passes its band; the assembled image on `home` (kc_comm_gather_bands).
pub fn gather_bands(band: &SlotImage, y0: i32, full_height: u32, home: i32) -> Result<Option<SlotImage>> {
    let mut out = ptr::null_mut();
    check(unsafe { kc_comm_gather_bands(band.raw(), y0, full_height, home, &mut out) })?;
    Ok(if out.is_null() { None } else { Some(wrap(out)) })
}

/// Rows [y0, y1) of `node`'s slot, bit-identical to those rows of the whole-image evaluation
/// (kc_live_graph_evaluate_band, csrc/bands.cpp): every rank takes its own band of the result.
pub fn evaluate_band(lg: *mut KcLiveGraph, node: NodeId, slot: SlotId, y0: i32, y1: i32) -> Result<SlotImage> {
    let mut out = ptr::null_mut();
    check(unsafe { kc_live_graph_evaluate_band(lg, node.0, slot.0, y0, y1, &mut out) })?;
    Ok(wrap(out))
}
