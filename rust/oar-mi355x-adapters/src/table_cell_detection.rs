//! `TableCellDetectionAdapter` (oar-ocr-core/src/domain/adapters/table_cell_detection_adapter.rs) with the model half on the GPU
//! (`oar_layout_*` with `model_type = 1 "rtdetr"`; no C symbols of its own).
//!
//! The reference adapter = `RTDetrModel::forward` (`DetResizeForTest` to the fixed `image_shape` with its default Triangle filter,
//! BGR tensor scaled by 1/255 without mean / std shift, graph with `image` + `scale_factor` + `im_shape`;
//! models/detection/rtdetr.rs:38-50, 86-112, 250-284) -> `LayoutPostProcess::apply` (model type "rtdetr", NMS 0.5,
//! `max_detections = max_cells`; :245-251) -> the adapter's per-call filter (`score < threshold` dropped, stop at `max_cells`;
//! :94-132).  The detection transformer's query selection (`TopK`, `GatherND`, `GatherElements`, tensor-indexed `Gather`) runs
//! inside the engine; everything up to `LayoutPostProcess`'s output is one C call, the per-call filter stays here.
//! Source-only, never compiled here (no Rust toolchain in the backend's build image): checked lexically by
//! tests/test_rust_bindings_cpu.py.

use crate::error::{Mi355xError, check};
use crate::ffi_util::{ImageBatch, device_id_from_ort_config, model_bytes, slice_or_empty};
use crate::layout_detection::LayoutHandle;
use oar_mi355x_sys as sys;
use oar_ocr_core::core::OCRError;
use oar_ocr_core::core::config::OrtSessionConfig;
use oar_ocr_core::core::inference::ModelSource;
use oar_ocr_core::core::traits::adapter::{AdapterBuilder, AdapterInfo, ModelAdapter, OrtConfigurable};
use oar_ocr_core::core::traits::task::{Task, TaskType};
use oar_ocr_core::domain::adapters::TableCellModelConfig;
use oar_ocr_core::domain::tasks::{TableCellDetection, TableCellDetectionConfig, TableCellDetectionOutput, TableCellDetectionTask};
use oar_ocr_core::processors::BoundingBox;
use std::ptr::NonNull;

struct CellResultGuard(sys::oar_layout_result);

impl Drop for CellResultGuard {
    fn drop(&mut self) {
        // SAFETY: filled by oar_layout_run or all-NULL.
        unsafe { sys::oar_layout_result_free(&mut self.0) }
    }
}

/// `TableCellDetectionAdapter` with resize, normalisation, the RT-DETR graph and `LayoutPostProcess` on the GPU.
#[derive(Debug)]
pub struct Mi355xTableCellDetectionAdapter {
    handle: LayoutHandle,
    info: AdapterInfo,
    model_config: TableCellModelConfig,
    config: TableCellDetectionConfig,
}

impl ModelAdapter for Mi355xTableCellDetectionAdapter {
    type Task = TableCellDetectionTask;

    fn info(&self) -> AdapterInfo {
        self.info.clone()
    }

    fn execute(
        &self,
        input: <Self::Task as Task>::Input,
        config: Option<&<Self::Task as Task>::Config>,
    ) -> Result<<Self::Task as Task>::Output, OCRError> {
        let effective_config = config.unwrap_or(&self.config);
        let batch_len = input.images.len();
        let images: Vec<&image::RgbImage> = input.images.iter().map(AsRef::as_ref).collect();
        let batch = ImageBatch::new(images.iter().copied());
        let mut result = CellResultGuard(sys::oar_layout_result {
            n_images: 0,
            n_boxes: 0,
            box_offsets: std::ptr::null_mut(),
            boxes: std::ptr::null_mut(),
            classes: std::ptr::null_mut(),
            scores: std::ptr::null_mut(),
            feature_dim: 0,
        });
        // SAFETY: three arrays of batch.len() entries; the page buffers outlive the call; result is a valid out-parameter.
        let status = unsafe {
            sys::oar_layout_run(self.handle.0.as_ptr(), batch.ptrs.as_ptr(), batch.widths.as_ptr(), batch.heights.as_ptr(), batch.len() as u32, &mut result.0)
        };
        check(status).map_err(|e| e.into_adapter_error("TableCellDetectionAdapter", format!("RTDetr forward (batch_size={batch_len})")))?;

        let r = &result.0;
        let (n, nb) = (r.n_images as usize, r.n_boxes as usize);
        // SAFETY: lengths as documented for oar_layout_result.
        let (offsets, boxes, classes, scores) = unsafe {
            (slice_or_empty(r.box_offsets, n + 1), slice_or_empty(r.boxes, nb * 4), slice_or_empty(r.classes, nb), slice_or_empty(r.scores, nb))
        };
        // the adapter's own filter (table_cell_detection_adapter.rs:103-129)
        let mut all_cells = Vec::with_capacity(n);
        for i in 0..n {
            let mut cells = Vec::new();
            for b in offsets[i] as usize..offsets[i + 1] as usize {
                let score = scores[b];
                if score < effective_config.score_threshold {
                    continue;
                }
                let label = self.model_config.class_labels.get(&(classes[b].max(0) as usize)).cloned().unwrap_or_else(|| "cell".to_string());
                cells.push(TableCellDetection { bbox: BoundingBox::from_coords(boxes[b * 4], boxes[b * 4 + 1], boxes[b * 4 + 2], boxes[b * 4 + 3]), score, label });
                if cells.len() >= effective_config.max_cells {
                    break;
                }
            }
            all_cells.push(cells);
        }
        Ok(TableCellDetectionOutput { cells: all_cells })
    }

    fn supports_batching(&self) -> bool {
        true
    }

    fn recommended_batch_size(&self) -> usize {
        4 // table_cell_detection_adapter.rs:175-177
    }
}

/// Builder with the surface of `TableCellDetectionAdapterBuilder` (table_cell_detection_adapter.rs:180-288).
#[derive(Debug, Clone)]
pub struct Mi355xTableCellDetectionAdapterBuilder {
    config: TableCellDetectionConfig,
    model_config: Option<TableCellModelConfig>,
    device_id: i32,
}

impl Default for Mi355xTableCellDetectionAdapterBuilder {
    fn default() -> Self {
        Self::new()
    }
}

impl Mi355xTableCellDetectionAdapterBuilder {
    /// The wired variant is the default, as `RTDetrTableCellAdapterBuilder::new` (:296-309).
    pub fn new() -> Self {
        Self { config: TableCellDetectionConfig::default(), model_config: Some(TableCellModelConfig::rtdetr_l_wired_table_cell_det()), device_id: 0 }
    }

    /// `RTDetrTableCellAdapterBuilder::wireless` (:311-317)
    pub fn wireless() -> Self {
        Self { config: TableCellDetectionConfig::default(), model_config: Some(TableCellModelConfig::rtdetr_l_wireless_table_cell_det()), device_id: 0 }
    }

    pub fn model_config(mut self, config: TableCellModelConfig) -> Self {
        self.model_config = Some(config);
        self
    }

    pub fn score_threshold(mut self, threshold: f32) -> Self {
        self.config.score_threshold = threshold;
        self
    }

    pub fn max_cells(mut self, max: usize) -> Self {
        self.config.max_cells = max;
        self
    }

    pub fn device_id(mut self, device_id: i32) -> Self {
        self.device_id = device_id;
        self
    }
}

impl AdapterBuilder for Mi355xTableCellDetectionAdapterBuilder {
    type Config = TableCellDetectionConfig;
    type Adapter = Mi355xTableCellDetectionAdapter;

    fn build(self, model_source: impl Into<ModelSource>) -> Result<Self::Adapter, OCRError> {
        let model_config = self.model_config.ok_or_else(|| OCRError::InvalidInput { message: "Table cell model configuration is required".to_string() })?;
        // TableCellDetectionConfig's derived validator (domain/tasks/table_cell_detection.rs:15-24)
        if !(0.0..=1.0).contains(&self.config.score_threshold) || self.config.max_cells < 1 {
            return Err(OCRError::ConfigError { message: "score_threshold must be in [0, 1] and max_cells >= 1".to_string() });
        }
        if model_config.model_type != "rtdetr" {
            return Err(OCRError::InvalidInput {
                message: format!("Unsupported model type '{}' for table cell detection. Supported type: rtdetr", model_config.model_type),
            });
        }
        let (input_h, input_w) = model_config.input_size.unwrap_or((640, 640));
        let source: ModelSource = model_source.into();
        let (bytes, shown) = model_bytes(&source)?;
        let cfg = sys::oar_layout_cfg {
            device_id: self.device_id,
            input_h,
            input_w,
            resize_filter: 0, // Triangle: DetResizeForTest's default, which RTDetrModel keeps (resize_detection.rs:100)
            color_bgr: 1,
            scale: 1.0 / 255.0,
            mean: [0.0f32, 0.0, 0.0],
            std: [1.0f32, 1.0, 1.0],
            num_classes: model_config.num_classes as u32,
            model_type: 1,
            score_threshold: self.config.score_threshold,
            nms_threshold: 0.5,
            max_detections: self.config.max_cells as u32,
        };
        let mut h: *mut sys::oar_layout = std::ptr::null_mut();
        // SAFETY: bytes is valid for bytes.len(); cfg and h are valid for the call.
        let status = unsafe { sys::oar_layout_create(bytes.as_ptr(), bytes.len(), &cfg, &mut h) };
        check(status).map_err(|e: Mi355xError| e.into_model_load(&shown))?;
        let handle = LayoutHandle(NonNull::new(h).ok_or_else(|| OCRError::ConfigError {
            message: "oar_layout_create returned a null handle".to_string(),
        })?);
        let info = AdapterInfo::new(
            format!("TableCellDetection_{}", model_config.model_name),
            TaskType::TableCellDetection,
            format!("Table cell detection adapter for {} with {} classes", model_config.model_name, model_config.num_classes),
        );
        Ok(Mi355xTableCellDetectionAdapter { handle, info, model_config, config: self.config })
    }

    fn with_config(mut self, config: Self::Config) -> Self {
        self.config = config;
        self
    }

    fn adapter_type(&self) -> &str {
        "RTDetrTableCell"
    }
}

/// `OrtConfigurable` (core/traits/adapter.rs:126-129): only the device ordinal applies.
impl OrtConfigurable for Mi355xTableCellDetectionAdapterBuilder {
    fn with_ort_config(mut self, config: OrtSessionConfig) -> Self {
        if let Some(device_id) = device_id_from_ort_config(&config) {
            self.device_id = device_id;
        }
        self
    }
}
