"""Operator / exchange layer around the record kernels (mirror of the reference's operator plugin API)."""
from .exchange_operator import NONE_AVAILABLE, NONE_LEFT, ExchangeOperator, RecordPool, RecordPoolError  # noqa: F401
from .record_handler import ExchangeRecord, RecordHandler, RecordHandlerError  # noqa: F401
from .tasks import (AggregateConfig, AggregateOperatorTask, AggregateTask, AggregateTaskBuilder, FilterConfig, FilterOperatorTask, FilterTask, FilterTaskBuilder, JoinConfig, JoinOperatorTask, JoinTask, JoinTaskBuilder, MaterializeFilesConfig,  # noqa: F401
                    MaterializeFilesOperatorTask, MaterializeFilesTask, MaterializeFilesTaskBuilder,
                    OperatorInstanceConfig, OperatorTaskRegistry, OperatorTaskRegistryError, OrderByConfig,
                    OrderByOperatorTask, OrderByTask, OrderByTaskBuilder, TaskBuilder, WindowConfig, WindowOperatorTask, WindowTask,
                    WindowTaskBuilder, build_default_operator_task_registry)
