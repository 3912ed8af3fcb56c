"""Operator tasks and the plugin API they register through.

Reference (OPS = src/handlers/operator_handler/operators):
  TaskBuilder trait                         OPS/traits.rs:22-36
  OperatorTaskRegistry                      OPS/operator_task_registry.rs:40-162
  FilterConfig / FilterTask / FilterTaskBuilder        OPS/filter_tasks/{config.rs, filter_task.rs:30-199}
  MaterializeFilesConfig / MaterializeFilesTask / ...  OPS/materialize_tasks/{config.rs, materialize_files_task.rs:30-230}
  OperatorTask::{Filter{expr}, MaterializeFiles{data_format, fields}}  src/planner/physical_planner.rs:58-65
  OrderByOperatorTask / OrderByTask         not in the reference (its DEV_NOTES.md lists ORDER BY as the next operator):
                                            a blocking single-instance sort over `record_utils.sort_records`
  AggregateOperatorTask / AggregateTask     not in the reference either: GROUP BY, a blocking single-instance aggregation
                                            over `record_utils.aggregate_records`
  WindowOperatorTask / WindowTask           not in the reference either: window functions (fn(...) OVER (...)), a blocking
                                            single-instance operator over `record_utils.window_records` + `project_record`
  JoinOperatorTask / JoinTask               not in the reference either: JOIN (inner, left, right, full, semi, anti), a blocking
                                            single-instance equi-join of two inbound exchanges over `record_utils.join_records`

The hot loops call `record_utils.filter_record` / `project_record` exactly where the reference does
(filter_task.rs:99, materialize_files_task.rs:110); here those are the HIP kernels.  The control plane around
them (message router, pipes, TCP) is out of scope: `build` receives the exchanges directly.
"""
from __future__ import annotations

import abc
import dataclasses
import os
import uuid
from typing import Any, Callable, List, Optional, Sequence

from .. import record_utils
from .. import sqlast as A
from .exchange_operator import ExchangeOperator
from .record_handler import RecordHandler


# ---- planner types the tasks consume ------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class FilterOperatorTask:
    """planner::OperatorTask::Filter { expr }"""
    expr: A.Expr

    def task_name(self) -> str:
        return "filter"


@dataclasses.dataclass(frozen=True)
class MaterializeFilesOperatorTask:
    """planner::OperatorTask::MaterializeFiles { data_format, fields }"""
    data_format: str
    fields: Sequence[A.SelectItem]

    def task_name(self) -> str:
        return "materialize_files"


@dataclasses.dataclass(frozen=True)
class ReadFilesOperatorTask:
    """planner::OperatorTask::TableFunc { alias, func_name: "read_files", args, max_rows_per_batch } with the path argument
    already parsed (ReadFilesConfig::parse_config, read_files_task.rs:66-107)"""
    path: str                       # glob below the connection's root
    alias: Optional[str] = None
    max_rows_per_batch: int = 10_000   # physical_planner.rs:323

    def task_name(self) -> str:
        return "read_files"


@dataclasses.dataclass(frozen=True)
class OrderByOperatorTask:
    """ORDER BY keys [LIMIT n] (the reference's planner has no such task yet; shaped like its siblings)"""
    order_by: Sequence[A.OrderByExpr]
    limit: Optional[int] = None
    max_rows_per_record: int = 10_000   # physical_planner.rs:323 (the records the read_files task sends)

    def task_name(self) -> str:
        return "order_by"


@dataclasses.dataclass(frozen=True)
class AggregateOperatorTask:
    """GROUP BY keys with the output items of the SELECT list (`sqlparse.aggregate_plan`); shaped like OrderByOperatorTask"""
    keys: Sequence[A.Expr]
    items: Sequence[A.AggItem]
    max_rows_per_record: int = 10_000

    def task_name(self) -> str:
        return "aggregate"


@dataclasses.dataclass(frozen=True)
class WindowOperatorTask:
    """One window specification with the items and the final projection of the SELECT list (`sqlparse.window_plan`); shaped
    like AggregateOperatorTask"""
    partition_by: Sequence[A.Expr]
    order_by: Sequence[A.OrderByExpr]
    items: Sequence[A.WindowItem]
    projection: Sequence[A.SelectItem]
    max_rows_per_record: int = 10_000

    def task_name(self) -> str:
        return "window"


@dataclasses.dataclass(frozen=True)
class JoinOperatorTask:
    """JOIN on the (left column, right column) pairs of the ON condition (`sqlparse.join_plan`); inbound exchange 0
    is the left input, 1 the right; shaped like AggregateOperatorTask.  `kind` is the `how` of `record_utils.join_records`."""
    keys: Sequence[Any]
    max_rows_per_record: int = 10_000
    kind: str = "inner"

    def task_name(self) -> str:
        return "join"


@dataclasses.dataclass
class OperatorInstanceConfig:
    """operator_handler_state.rs:28-35 (fields the tasks use)"""
    instance_id: int
    operator_id: str
    query_id: int
    task: Any
    device_id: int = 0


# ---- plugin API ------------------------------------------------------------------------------------------
class TaskBuilder(abc.ABC):
    """OPS/traits.rs:22-36.  `build` returns a callable that runs the task to completion and returns None on
    success or the error (the reference sends that through a oneshot channel)."""

    @abc.abstractmethod
    def build(self, op_in_config: OperatorInstanceConfig, inbound_exchanges: List[ExchangeOperator],
              outbound_exchange: Optional[ExchangeOperator]) -> Callable[[], Optional[Exception]]:
        ...


class OperatorTaskRegistryError(Exception):
    pass


class OperatorTaskRegistry:
    def __init__(self):
        self.filter_task: Optional[TaskBuilder] = None
        self.materialize_files_task: Optional[TaskBuilder] = None
        self.materialize_data_formats: List[str] = []
        self.table_func_tasks: dict = {}
        self.order_by_task: Optional[TaskBuilder] = None
        self.aggregate_task: Optional[TaskBuilder] = None
        self.join_task: Optional[TaskBuilder] = None
        self.window_task: Optional[TaskBuilder] = None

    def add_filter_task_builder(self, builder: TaskBuilder) -> "OperatorTaskRegistry":
        if self.filter_task is not None:
            raise OperatorTaskRegistryError("filter task builder already set")
        self.filter_task = builder
        return self

    def add_materialize_files_builder(self, builder: TaskBuilder, data_formats: List[str]) -> "OperatorTaskRegistry":
        if self.materialize_files_task is not None:
            raise OperatorTaskRegistryError("materialize file task builder already set")
        self.materialize_files_task = builder
        self.materialize_data_formats = list(data_formats)
        return self

    def add_table_func_task_builder(self, func_name: str, builder: TaskBuilder) -> "OperatorTaskRegistry":
        """operator_task_registry.rs:35-49 (the syntax validator is the planner's business: out of scope)"""
        if func_name in self.table_func_tasks:
            raise OperatorTaskRegistryError(f"table func task builder for {func_name} already set")
        self.table_func_tasks[func_name] = builder
        return self

    def add_order_by_task_builder(self, builder: TaskBuilder) -> "OperatorTaskRegistry":
        if self.order_by_task is not None:
            raise OperatorTaskRegistryError("order by task builder already set")
        self.order_by_task = builder
        return self

    def add_aggregate_task_builder(self, builder: TaskBuilder) -> "OperatorTaskRegistry":
        if self.aggregate_task is not None:
            raise OperatorTaskRegistryError("aggregate task builder already set")
        self.aggregate_task = builder
        return self

    def add_window_task_builder(self, builder: TaskBuilder) -> "OperatorTaskRegistry":
        if self.window_task is not None:
            raise OperatorTaskRegistryError("window task builder already set")
        self.window_task = builder
        return self

    def add_join_task_builder(self, builder: TaskBuilder) -> "OperatorTaskRegistry":
        if self.join_task is not None:
            raise OperatorTaskRegistryError("join task builder already set")
        self.join_task = builder
        return self

    def find_task_builder(self, task) -> Optional[TaskBuilder]:
        if isinstance(task, ReadFilesOperatorTask):
            return self.table_func_tasks.get("read_files")
        if isinstance(task, FilterOperatorTask):
            return self.filter_task
        if isinstance(task, OrderByOperatorTask):
            return self.order_by_task
        if isinstance(task, AggregateOperatorTask):
            return self.aggregate_task
        if isinstance(task, JoinOperatorTask):
            return self.join_task
        if isinstance(task, WindowOperatorTask):
            return self.window_task
        if isinstance(task, MaterializeFilesOperatorTask):
            if task.data_format in self.materialize_data_formats:
                return self.materialize_files_task
        return None


# ---- filter --------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class FilterConfig:
    expr: A.Expr

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "FilterConfig":
        if not isinstance(op_in_config.task, FilterOperatorTask):
            raise ValueError("operator instance config is not a filter task")
        return FilterConfig(op_in_config.task.expr)


class FilterTask:
    """filter_task.rs:65-142.  `group_size` > 1 is the GPU extension: the task drains up to that many queued records
    of one schema and filters them with ONE kernel launch (`record_utils.filter_records`); every output still
    carries its input record id and is acked individually, so the exchange protocol is unchanged."""

    def __init__(self, op_in_config: OperatorInstanceConfig, filter_config: FilterConfig,
                 inbound_exchanges, outbound_exchange, filter_fn=None, ctx=None, group_size: int = 1):
        self.operator_instance_config = op_in_config
        self.filter_config = filter_config
        self.inbound_exchanges = inbound_exchanges
        self.outbound_exchange = outbound_exchange
        self._filter = filter_fn
        self._ctx = ctx
        self.group_size = max(1, int(group_size))
        self.records_processed = 0
        self.rows_in = 0
        self.rows_out = 0
        self.group_calls = 0

    def _context(self):
        if self._ctx is None:
            self._ctx = record_utils.Context(self.operator_instance_config.device_id)
        return self._ctx

    def _filter_record(self, rec, aliases):
        if self._filter is not None:
            return self._filter(rec, aliases, self.filter_config.expr)
        return record_utils.filter_record(rec, aliases, self.filter_config.expr, ctx=self._context())

    def _filter_group(self, group):
        """one library call for records that share schema, residency and table aliases; else record by record"""
        first = group[0]
        same = self._filter is None and len(group) > 1 and all(
            g.table_aliases == first.table_aliases and type(g.record) is type(first.record) and
            _schema_of(g.record) == _schema_of(first.record) for g in group[1:])
        if not same:
            return [self._filter_record(g.record, g.table_aliases) for g in group]
        self.group_calls += 1
        return record_utils.filter_records([g.record for g in group], first.table_aliases, self.filter_config.expr,
                                           ctx=self._context())

    def async_main(self) -> None:
        """filter_task.rs:65-142: pull -> filter -> push (same record id) -> ack"""
        rec_handler = RecordHandler.initiate(self.operator_instance_config, self.inbound_exchanges, self.outbound_exchange)
        try:   # an error ends the task (filter_task.rs `?`): its heartbeats must stop with it, so the exchange requeues
            while True:
                exchange_rec = rec_handler.next_record()
                if exchange_rec is None:
                    break
                group = [exchange_rec]
                while len(group) < self.group_size:
                    more = rec_handler.try_next_record()
                    if more is None:
                        break
                    group.append(more)
                for exchange_rec, filtered_rec in zip(group, self._filter_group(group)):
                    rec_handler.send_record_to_outbound_exchange(exchange_rec.record_id, filtered_rec, exchange_rec.table_aliases)
                    rec_handler.complete_record(exchange_rec)
                    self.records_processed += 1
                    self.rows_in += exchange_rec.record.num_rows
                    self.rows_out += filtered_rec.num_rows
        finally:
            rec_handler.close()


def _schema_of(rec):
    if hasattr(rec, "schema"):
        return rec.schema
    return tuple(zip(rec.column_names, rec.column_formats))


class FilterTaskBuilder(TaskBuilder):
    """The GPU filter operator. Swap it in with `OperatorTaskRegistry.add_filter_task_builder` -- the planner's
    DAG and the exchanges are untouched (operator_task_registry.rs:51-57)."""

    def __init__(self, filter_fn=None, group_size: int = 1):
        self._filter_fn = filter_fn
        self._group_size = group_size

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        task = FilterTask(op_in_config, FilterConfig.try_from(op_in_config), inbound_exchanges, outbound_exchange,
                          filter_fn=self._filter_fn, group_size=self._group_size)

        def run():
            try:
                task.async_main()
                return None
            except Exception as err:   # noqa: BLE001 -- any error ends the instance (producer_operator.rs:179-183)
                return err

        run.task = task
        return run


# ---- order by ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class OrderByConfig:
    order_by: Sequence[A.OrderByExpr]
    limit: Optional[int] = None
    max_rows_per_record: int = 10_000

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "OrderByConfig":
        t = op_in_config.task
        if not isinstance(t, OrderByOperatorTask):
            raise ValueError("operator instance config is not an order by task")
        if not t.order_by:
            raise ValueError("an order by task needs at least one key")
        if t.max_rows_per_record < 1:
            raise ValueError("max_rows_per_record must be at least 1")
        return OrderByConfig(tuple(t.order_by), t.limit, t.max_rows_per_record)


class OrderByTask:
    """A blocking, single-instance operator: pulls every inbound record (each tracked and heart-beaten by the
    RecordHandler while it is held), sorts them all with ONE `sort_records` call, sends the result cut into records of
    at most `max_rows_per_record` rows with record ids 0, 1, 2, ... in sorted order, and only then acks its inputs --
    if anything fails before that, the exchange requeues them (the ack-after-send rule of FilterTask).  `sort_fn(records,
    table_aliases, order_by, limit)` replaces the library call (tests on the CPU)."""

    def __init__(self, op_in_config: OperatorInstanceConfig, config: OrderByConfig, inbound_exchanges, outbound_exchange,
                 sort_fn=None, ctx=None):
        self.operator_instance_config = op_in_config
        self.config = config
        self.inbound_exchanges = inbound_exchanges
        self.outbound_exchange = outbound_exchange
        self._sort = sort_fn
        self._ctx = ctx
        self.rows_in = 0
        self.rows_out = 0
        self.records_sent = 0

    def _context(self):
        if self._ctx is None:
            self._ctx = record_utils.Context(self.operator_instance_config.device_id)
        return self._ctx

    def _sort_records(self, records, aliases):
        if self._sort is not None:
            return self._sort(records, aliases, self.config.order_by, self.config.limit)
        return record_utils.sort_records(records, aliases, self.config.order_by, limit=self.config.limit, ctx=self._context())

    def async_main(self) -> None:
        rec_handler = RecordHandler.initiate(self.operator_instance_config, self.inbound_exchanges, self.outbound_exchange)
        try:
            held = []
            while True:
                exchange_rec = rec_handler.next_record_to_hold()
                if exchange_rec is None:
                    break
                held.append(exchange_rec)
            if not held:
                return
            self.rows_in = sum(h.record.num_rows for h in held)
            aliases = held[0].table_aliases
            result = self._sort_records([h.record for h in held], aliases)
            n, step = result.num_rows, self.config.max_rows_per_record
            for record_id, start in enumerate(range(0, max(n, 1), step)):
                rec_handler.send_record_to_outbound_exchange(record_id, result.slice(start, min(step, n - start)), aliases)
                self.records_sent += 1
            self.rows_out = n
            for h in held:
                rec_handler.complete_record(h)
        finally:
            rec_handler.close()


class OrderByTaskBuilder(TaskBuilder):
    def __init__(self, sort_fn=None):
        self._sort_fn = sort_fn

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        task = OrderByTask(op_in_config, OrderByConfig.try_from(op_in_config), inbound_exchanges, outbound_exchange,
                           sort_fn=self._sort_fn)

        def run():
            try:
                task.async_main()
                return None
            except Exception as err:   # noqa: BLE001 -- any error ends the instance
                return err

        run.task = task
        return run


# ---- group by ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class AggregateConfig:
    keys: Sequence[A.Expr]
    items: Sequence[A.AggItem]
    max_rows_per_record: int = 10_000

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "AggregateConfig":
        t = op_in_config.task
        if not isinstance(t, AggregateOperatorTask):
            raise ValueError("operator instance config is not an aggregate task")
        if not t.items:
            raise ValueError("an aggregate task needs at least one output item")
        if t.max_rows_per_record < 1:
            raise ValueError("max_rows_per_record must be at least 1")
        return AggregateConfig(tuple(t.keys), tuple(t.items), t.max_rows_per_record)


class AggregateTask:
    """A blocking, single-instance operator with the protocol of OrderByTask: pulls and holds every inbound record,
    aggregates them all with ONE `aggregate_records` call, sends the groups (in key order) cut into records of at most
    `max_rows_per_record` rows with record ids 0, 1, 2, ..., and only then acks its inputs.  When no record came in nothing
    is sent, also without a GROUP BY key: there is no schema to aggregate over.
    `aggregate_fn(records, table_aliases, keys, items)` replaces the library call (tests on the CPU)."""

    def __init__(self, op_in_config: OperatorInstanceConfig, config: AggregateConfig, inbound_exchanges, outbound_exchange,
                 aggregate_fn=None, ctx=None):
        self.operator_instance_config = op_in_config
        self.config = config
        self.inbound_exchanges = inbound_exchanges
        self.outbound_exchange = outbound_exchange
        self._aggregate = aggregate_fn
        self._ctx = ctx
        self.rows_in = 0
        self.rows_out = 0
        self.records_sent = 0

    def _context(self):
        if self._ctx is None:
            self._ctx = record_utils.Context(self.operator_instance_config.device_id)
        return self._ctx

    def _aggregate_records(self, records, aliases):
        if self._aggregate is not None:
            return self._aggregate(records, aliases, self.config.keys, self.config.items)
        return record_utils.aggregate_records(records, aliases, self.config.keys, self.config.items, ctx=self._context())

    def async_main(self) -> None:
        rec_handler = RecordHandler.initiate(self.operator_instance_config, self.inbound_exchanges, self.outbound_exchange)
        try:
            held = []
            while True:
                exchange_rec = rec_handler.next_record_to_hold()
                if exchange_rec is None:
                    break
                held.append(exchange_rec)
            if not held:
                return
            self.rows_in = sum(h.record.num_rows for h in held)
            result = self._aggregate_records([h.record for h in held], held[0].table_aliases)
            out_aliases = [[] for _ in range(result.num_columns)]   # the output columns are new: no table prefix reaches them
            n, step = result.num_rows, self.config.max_rows_per_record
            for record_id, start in enumerate(range(0, max(n, 1), step)):
                rec_handler.send_record_to_outbound_exchange(record_id, result.slice(start, min(step, n - start)), out_aliases)
                self.records_sent += 1
            self.rows_out = n
            for h in held:
                rec_handler.complete_record(h)
        finally:
            rec_handler.close()


class AggregateTaskBuilder(TaskBuilder):
    def __init__(self, aggregate_fn=None):
        self._aggregate_fn = aggregate_fn

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        task = AggregateTask(op_in_config, AggregateConfig.try_from(op_in_config), inbound_exchanges, outbound_exchange,
                             aggregate_fn=self._aggregate_fn)

        def run():
            try:
                task.async_main()
                return None
            except Exception as err:   # noqa: BLE001 -- any error ends the instance
                return err

        run.task = task
        return run


# ---- window functions -----------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class WindowConfig:
    partition_by: Sequence[A.Expr]
    order_by: Sequence[A.OrderByExpr]
    items: Sequence[A.WindowItem]
    projection: Sequence[A.SelectItem]
    max_rows_per_record: int = 10_000

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "WindowConfig":
        t = op_in_config.task
        if not isinstance(t, WindowOperatorTask):
            raise ValueError("operator instance config is not a window task")
        if not t.items:
            raise ValueError("a window task needs at least one item")
        if not t.projection:
            raise ValueError("a window task needs at least one projected field")
        if t.max_rows_per_record < 1:
            raise ValueError("max_rows_per_record must be at least 1")
        return WindowConfig(tuple(t.partition_by), tuple(t.order_by), tuple(t.items), tuple(t.projection), t.max_rows_per_record)


class WindowTask:
    """A blocking, single-instance operator with the protocol of AggregateTask: pulls and holds every inbound record,
    evaluates every window item with ONE `window_records` call (the rows come back in input order: record order, then row
    order), finishes the SELECT list with ONE `project_record` over that result, sends it cut into records of at most
    `max_rows_per_record` rows with record ids 0, 1, 2, ..., and only then acks its inputs.  When no record came in nothing
    is sent.  `window_fn(records, table_aliases, partition_by, order_by, items)` and `project_fn(fields, record,
    table_aliases)` replace the library calls (tests on the CPU)."""

    def __init__(self, op_in_config: OperatorInstanceConfig, config: WindowConfig, inbound_exchanges, outbound_exchange,
                 window_fn=None, project_fn=None, ctx=None):
        self.operator_instance_config = op_in_config
        self.config = config
        self.inbound_exchanges = inbound_exchanges
        self.outbound_exchange = outbound_exchange
        self._window = window_fn
        self._project = project_fn
        self._ctx = ctx
        self.rows_in = 0
        self.rows_out = 0
        self.records_sent = 0

    def _context(self):
        if self._ctx is None:
            self._ctx = record_utils.Context(self.operator_instance_config.device_id)
        return self._ctx

    def _window_records(self, records, aliases):
        c = self.config
        if self._window is not None:
            return self._window(records, aliases, c.partition_by, c.order_by, c.items)
        return record_utils.window_records(records, aliases, c.partition_by, c.order_by, c.items, ctx=self._context())

    def _project_record(self, rec, aliases):
        if self._project is not None:
            return self._project(self.config.projection, rec, aliases)
        return record_utils.project_record(self.config.projection, rec, aliases, ctx=self._context())

    def async_main(self) -> None:
        rec_handler = RecordHandler.initiate(self.operator_instance_config, self.inbound_exchanges, self.outbound_exchange)
        try:
            held = []
            while True:
                exchange_rec = rec_handler.next_record_to_hold()
                if exchange_rec is None:
                    break
                held.append(exchange_rec)
            if not held:
                return
            self.rows_in = sum(h.record.num_rows for h in held)
            aliases = held[0].table_aliases
            windowed = self._window_records([h.record for h in held], aliases)
            # the item columns are new: no table prefix reaches them
            win_aliases = None if aliases is None else list(aliases) + [[] for _ in range(windowed.num_columns - len(aliases))]
            result = self._project_record(windowed, win_aliases)
            out_aliases = [[] for _ in range(result.num_columns)]
            n, step = result.num_rows, self.config.max_rows_per_record
            for record_id, start in enumerate(range(0, max(n, 1), step)):
                rec_handler.send_record_to_outbound_exchange(record_id, result.slice(start, min(step, n - start)), out_aliases)
                self.records_sent += 1
            self.rows_out = n
            for h in held:
                rec_handler.complete_record(h)
        finally:
            rec_handler.close()


class WindowTaskBuilder(TaskBuilder):
    def __init__(self, window_fn=None, project_fn=None):
        self._window_fn = window_fn
        self._project_fn = project_fn

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        task = WindowTask(op_in_config, WindowConfig.try_from(op_in_config), inbound_exchanges, outbound_exchange,
                          window_fn=self._window_fn, project_fn=self._project_fn)

        def run():
            try:
                task.async_main()
                return None
            except Exception as err:   # noqa: BLE001 -- any error ends the instance
                return err

        run.task = task
        return run


# ---- join ---------------------------------------------------------------------------------------------------------------
JOIN_KINDS = ("inner", "left", "right", "full", "semi", "anti")


@dataclasses.dataclass(frozen=True)
class JoinConfig:
    keys: Sequence[Any]
    max_rows_per_record: int = 10_000
    kind: str = "inner"

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "JoinConfig":
        t = op_in_config.task
        if not isinstance(t, JoinOperatorTask):
            raise ValueError("operator instance config is not a join task")
        if not t.keys:
            raise ValueError("a join task needs at least one pair of key columns")
        if t.max_rows_per_record < 1:
            raise ValueError("max_rows_per_record must be at least 1")
        if t.kind not in JOIN_KINDS:
            raise ValueError(f"a join task's kind must be one of {', '.join(JOIN_KINDS)}, not {t.kind!r}")
        return JoinConfig(tuple((l, r) for l, r in t.keys), t.max_rows_per_record, t.kind)


class JoinTask:
    """A blocking, single-instance operator with the protocol of AggregateTask over TWO inbound exchanges (0: the left input,
    1: the right): pulls and holds every record of both sides, joins them with ONE `join_records` call, sends the result
    (in the row order of its kind; inner: ascending by left row, then by right row) cut into records of at most
    `max_rows_per_record` rows with record ids 0, 1, 2, ... under the table aliases of the left columns followed by those of
    the right columns (semi and anti: the left columns only), and only then acks both sides.  When either side delivered no
    record nothing is sent, whatever the kind: there is no schema to join or to pad with.
    Each side has a RecordHandler of its own: a handler reads only its first exchange and tracks by record id, which the two
    exchanges may share.
    `join_fn(left_records, left_aliases, right_records, right_aliases, keys)` replaces the library call (tests on the CPU);
    for a kind other than "inner" it is called with `kind=` as a keyword on top."""

    def __init__(self, op_in_config: OperatorInstanceConfig, config: JoinConfig, inbound_exchanges, outbound_exchange,
                 join_fn=None, ctx=None):
        if len(inbound_exchanges) != 2:
            raise ValueError(f"a join task takes two inbound exchanges (left, right), not {len(inbound_exchanges)}")
        self.operator_instance_config = op_in_config
        self.config = config
        self.inbound_exchanges = inbound_exchanges
        self.outbound_exchange = outbound_exchange
        self._join = join_fn
        self._ctx = ctx
        self.rows_in = 0
        self.rows_out = 0
        self.records_sent = 0

    def _context(self):
        if self._ctx is None:
            self._ctx = record_utils.Context(self.operator_instance_config.device_id)
        return self._ctx

    def _join_records(self, left, left_aliases, right, right_aliases):
        kind = self.config.kind
        if self._join is not None:
            if kind == "inner":
                return self._join(left, left_aliases, right, right_aliases, self.config.keys)
            return self._join(left, left_aliases, right, right_aliases, self.config.keys, kind=kind)
        return record_utils.join_records(left, left_aliases, right, right_aliases, self.config.keys, ctx=self._context(), how=kind)

    def async_main(self) -> None:
        handlers = [RecordHandler.initiate(self.operator_instance_config, [ex], self.outbound_exchange) for ex in self.inbound_exchanges]
        try:
            held = [[], []]
            for side, handler in enumerate(handlers):
                while True:
                    exchange_rec = handler.next_record_to_hold()
                    if exchange_rec is None:
                        break
                    held[side].append(exchange_rec)
            self.rows_in = sum(h.record.num_rows for side in held for h in side)
            if held[0] and held[1]:
                left_aliases, right_aliases = held[0][0].table_aliases, held[1][0].table_aliases
                result = self._join_records([h.record for h in held[0]], left_aliases, [h.record for h in held[1]], right_aliases)
                out_aliases = [list(a) for a in left_aliases]
                if self.config.kind not in ("semi", "anti"):
                    out_aliases += [list(a) for a in right_aliases]
                n, step = result.num_rows, self.config.max_rows_per_record
                for record_id, start in enumerate(range(0, max(n, 1), step)):
                    handlers[0].send_record_to_outbound_exchange(record_id, result.slice(start, min(step, n - start)), out_aliases)
                    self.records_sent += 1
                self.rows_out = n
            for side, handler in enumerate(handlers):
                for h in held[side]:
                    handler.complete_record(h)
        finally:
            for handler in handlers:
                handler.close()


class JoinTaskBuilder(TaskBuilder):
    def __init__(self, join_fn=None):
        self._join_fn = join_fn

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        task = JoinTask(op_in_config, JoinConfig.try_from(op_in_config), inbound_exchanges, outbound_exchange, join_fn=self._join_fn)

        def run():
            try:
                task.async_main()
                return None
            except Exception as err:   # noqa: BLE001 -- any error ends the instance
                return err

        run.task = task
        return run


# ---- read_files (the table function in front of the path) -----------------------------------------------------
class ReadFilesTask:
    """read_files_task.rs:129-291 with `read_records` (:233-282) on the GPU: every matching Parquet file is opened through a
    RANGE reader (the footer, then exactly the chunks that are decoded -- the reference reads through opendal ranges), its row
    groups are decoded in HBM (`chq_parquet_read_columns`) and forwarded as device-resident records cut into zero-copy slices
    of `max_rows_per_batch` rows; `columns` prunes the scan (the reference's DEV_NOTES.md:123).  Files the decoder refuses
    (status 30: ZSTD, nested columns, ...) are read with pyarrow on the host -- the stand-in for the parquet crate."""

    def __init__(self, op_in_config: OperatorInstanceConfig, task: ReadFilesOperatorTask, storage_root: str, outbound_exchange,
                 ctx=None, columns: Optional[Sequence[str]] = None, device_records: bool = True):
        self.operator_instance_config = op_in_config
        self.config = task
        self.storage_root = storage_root
        self.outbound_exchange = outbound_exchange
        self._ctx = ctx
        self.columns = list(columns) if columns is not None else None
        self.device_records = device_records
        self.record_id = 0
        self.files_read: List[str] = []
        self.bytes_fetched = 0
        self.host_fallbacks = 0

    def _context(self):
        if self._ctx is None:
            self._ctx = record_utils.Context(self.operator_instance_config.device_id)
        return self._ctx

    def _send(self, rec_handler, record) -> None:
        aliases = record_utils.get_record_table_aliases(self.config.alias, record)
        rec_handler.send_record_to_outbound_exchange(self.record_id, record, aliases)
        self.record_id += 1

    def _read_records(self, rec_handler, path: str) -> None:
        size = os.path.getsize(path)
        step = max(1, int(self.config.max_rows_per_batch))
        with open(path, "rb") as fh:
            def read(offset: int, length: int) -> bytes:
                self.bytes_fetched += length
                return os.pread(fh.fileno(), length, offset)
            try:
                pf = record_utils.ParquetFile(None, reader=read, size=size)
            except record_utils.ChqError as err:
                if err.code != 30:
                    raise
                pf = None
            groups = None
            if pf is not None:
                try:
                    groups = pf.read_row_groups(ctx=self._context(), device_result=self.device_records, columns=self.columns)
                except record_utils.ChqError as err:
                    if err.code != 30:
                        raise
                finally:
                    pf.close()
        if groups is None:   # outside the GPU decoder's scope: the host reader, same batch size
            import pyarrow.parquet as pq
            self.host_fallbacks += 1
            for rec in pq.ParquetFile(path).iter_batches(batch_size=step, columns=self.columns):
                self._send(rec_handler, rec)
            return
        for group in groups:
            n = group.num_rows
            if n <= step:
                self._send(rec_handler, group)
                continue
            for at in range(0, n, step):
                self._send(rec_handler, group.slice(at, min(step, n - at)))

    def async_main(self) -> None:
        import glob
        rec_handler = RecordHandler.initiate(self.operator_instance_config, [], self.outbound_exchange)
        try:
            for path in sorted(glob.glob(os.path.join(self.storage_root, self.config.path.lstrip("/")), recursive=True)):
                self._read_records(rec_handler, path)
                self.files_read.append(path)
        finally:
            rec_handler.close()


class ReadFilesTaskBuilder(TaskBuilder):
    """The GPU read_files table function (`rust/gpu_read_files_task.rs` is the same task for the reference's registry)."""

    def __init__(self, storage_root: str, columns: Optional[Sequence[str]] = None, device_records: bool = True):
        self._root = storage_root
        self._columns = columns
        self._device_records = device_records

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        if not isinstance(op_in_config.task, ReadFilesOperatorTask):
            raise ValueError("operator instance config is not a read_files task")
        task = ReadFilesTask(op_in_config, op_in_config.task, self._root, outbound_exchange, columns=self._columns,
                             device_records=self._device_records)

        def run():
            try:
                task.async_main()
                return None
            except Exception as err:   # noqa: BLE001
                return err

        run.task = task
        return run


# ---- materialize ----------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class MaterializeFilesConfig:
    data_format: str
    fields: Sequence[A.SelectItem]

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "MaterializeFilesConfig":
        if not isinstance(op_in_config.task, MaterializeFilesOperatorTask):
            raise ValueError("operator instance config is not a materialize files task")
        return MaterializeFilesConfig(op_in_config.task.data_format, op_in_config.task.fields)


class MaterializeFilesTask:
    def __init__(self, op_in_config, config: MaterializeFilesConfig, inbound_exchanges, outbound_exchange,
                 storage_root: str, project_fn=None, ctx=None):
        self.operator_instance_config = op_in_config
        self.materialize_file_config = config
        self.inbound_exchanges = inbound_exchanges
        self.outbound_exchange = outbound_exchange
        self.storage_root = storage_root
        self._project = project_fn
        self._ctx = ctx
        self.files_written: List[str] = []

    def _project_record(self, rec, aliases):
        if self._project is not None:
            return self._project(self.materialize_file_config.fields, rec, aliases)
        if self._ctx is None:
            self._ctx = record_utils.Context(self.operator_instance_config.device_id)
        # the projected batch stays in HBM: the Parquet pages are encoded there too
        return record_utils.project_record(self.materialize_file_config.fields, rec, aliases, ctx=self._ctx, device_result=True)

    def _write_parquet(self, proj_rec, path: str) -> None:
        """materialize_files_task.rs:128-141 (AsyncArrowWriter ... write ... close).  A device-resident result is encoded on
        the GPU (`chq_record_to_parquet`) and only the finished file image reaches the host; column types that encoder does
        not write (and host-resident results, e.g. from an injected `project_fn`) go through pyarrow's writer."""
        import pyarrow as pa
        import pyarrow.parquet as pq
        if isinstance(proj_rec, record_utils.DeviceRecordBatch):
            try:
                image = record_utils.record_to_parquet(proj_rec, ctx=self._ctx, copy=False)
            except record_utils.ChqError as e:
                if e.code != 30:   # NotSupported: a type outside Int32/Int64/Float32/Float64/Boolean/Utf8
                    raise
                proj_rec = proj_rec.to_host()
            else:
                try:
                    with open(path, "wb") as f:
                        f.write(image.view)     # straight out of the library's host buffer
                finally:
                    image.release()
                return
        pq.write_table(pa.Table.from_batches([proj_rec]), path)

    def async_main(self) -> None:
        """materialize_files_task.rs:68-170: pull -> project -> write /query_results/<uuid>/rec_<id>.parquet -> ack."""
        rec_handler = RecordHandler.initiate(self.operator_instance_config, self.inbound_exchanges, self.outbound_exchange)
        query_uuid = uuid.UUID(int=self.operator_instance_config.query_id)
        out_dir = os.path.join(self.storage_root, "query_results", str(query_uuid))
        os.makedirs(out_dir, exist_ok=True)
        try:
            while True:
                exchange_rec = rec_handler.next_record()
                if exchange_rec is None:
                    break
                proj_rec = self._project_record(exchange_rec.record, exchange_rec.table_aliases)
                path = os.path.join(out_dir, f"rec_{exchange_rec.record_id}.parquet")
                self._write_parquet(proj_rec, path)
                self.files_written.append(path)
                rec_handler.complete_record(exchange_rec)
        finally:
            rec_handler.close()


class MaterializeFilesTaskBuilder(TaskBuilder):
    def __init__(self, storage_root: str, project_fn=None):
        self.storage_root = storage_root
        self._project_fn = project_fn

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        task = MaterializeFilesTask(op_in_config, MaterializeFilesConfig.try_from(op_in_config), inbound_exchanges,
                                    outbound_exchange, self.storage_root, project_fn=self._project_fn)

        def run():
            try:
                task.async_main()
                return None
            except Exception as err:   # noqa: BLE001
                return err

        run.task = task
        return run


def build_default_operator_task_registry(storage_root: str) -> OperatorTaskRegistry:
    """operator_task_registry.rs:150-162 with the GPU builders swapped in."""
    return (OperatorTaskRegistry()
            .add_table_func_task_builder("read_files", ReadFilesTaskBuilder(storage_root))
            .add_filter_task_builder(FilterTaskBuilder())
            .add_order_by_task_builder(OrderByTaskBuilder())
            .add_aggregate_task_builder(AggregateTaskBuilder())
            .add_window_task_builder(WindowTaskBuilder())
            .add_join_task_builder(JoinTaskBuilder())
            .add_materialize_files_builder(MaterializeFilesTaskBuilder(storage_root), ["parquet"]))
